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
// the shared positions of a call (bn254_pairing_check_batch_shared): mask 0 is the all-variable entry.  prepared: popcount(mask) records of BN254_G2_PREPARED_LEN
// bytes -- host memory in the host entries, device memory in the enqueue
struct PbShared {
  unsigned mask = 0; const uint8_t* prepared = nullptr;
  size_t count() const { return (size_t)__builtin_popcount(mask); }
  size_t bytes() const { return count() * PB_PREP_LEN; }
};
#pragma GCC visibility push(hidden)
PbDev* pb_dev(int device);
// BN254_E_BAD_ARG before any device is touched; *done: n == 0, nothing to do.  host_records: sh.prepared is host memory, so the headers of its records are checked too
int pb_check_args(const void* pairs, size_t item_stride, size_t n_pairs, size_t n, const void* status, const void* out_gt, bool wants_gt, bool* done,
                  const PbShared& sh = PbShared(), bool host_records = false);
// items per pass of a host entry whose staged item takes rec bytes behind lead bytes of records; items a reservation of n allocates workspace for
size_t pb_host_pass_of(size_t rec, size_t lead, size_t n);
size_t pb_ws_items_of(size_t n);
// caller holds d.mu: the device made ready (self-test at its first use) and the workspace grown to what a reservation of n items holds
int pb_ensure(PbDev& d, int device, size_t n);
// the form a launch of n items of n_pairs pairs takes under bn254_set_pairing_params, and the launch counted for bn254_pairing_state
int pb_form(size_t n_pairs, size_t n);
void pb_count_launch(int form);
#pragma GCC visibility pop
