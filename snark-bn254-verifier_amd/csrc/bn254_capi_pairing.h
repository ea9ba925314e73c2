// bn254_capi_pairing.h -- the per-DEVICE state of the pairing batch (bn254_capi_pairing.hip) for the entries that share it: the workspace, its lock and the completion
// event of the last call.  bn254_capi_kzg.hip runs on the same workspace, so a KZG call and a pairing call on one device serialise.
#pragma once
#include "bn254_capi_internal.h"
#include "bn254_pairing_batch.h"

struct PbDev {
  std::mutex mu;                       // uploads, (re)allocation, the enqueue of a call; held for the whole of a host-buffer call (the staging belongs to one call at a time)
  bool ready = false;
  DevBuf<int32_t> ws, one;             // G16_WS_BYTES_PER_PROOF per item; 1 in GT
  size_t ws_items() const { return ws.cap() / (size_t)(G16_WS_BYTES_PER_PROOF / 4); }
  Event busy_ev; bool busy_valid = false;
  // host-buffer entries: the records, status bytes and GT values of a pass on both sides
  Stream stream;
  DevBuf<uint8_t> d_in, d_status, d_gt;
  PinBuf<uint8_t> h_in, h_status, h_gt;
};
#pragma GCC visibility push(hidden)
PbDev* pb_dev(int device);
// caller holds d.mu: the device made ready (self-test at its first use) and the workspace grown to what a reservation of n items holds
int pb_ensure(PbDev& d, int device, size_t n);
// the form a launch of n items of n_pairs pairs takes under bn254_set_pairing_params, and the launch counted for bn254_pairing_state
int pb_form(size_t n_pairs, size_t n);
void pb_count_launch(int form);
#pragma GCC visibility pop
