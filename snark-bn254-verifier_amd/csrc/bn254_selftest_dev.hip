// bn254_selftest_dev.hip -- the device half of the self-test (bn254_selftest.h; include/bn254_verify.h, bn254_device_selftest): one function per check, each a few calls
// of the launchers the product and its probes use (bn254_kernels.h), on a stream of its own.  No kernel and no arithmetic here: what is under test is what the library
// ships.  Inputs travel in one pinned block, outputs come back in another; the only wait is on the stream.
#include "bn254_selftest.h"

using namespace bn254st;

namespace {
constexpr size_t WS_PROOFS = 256;                       // the workspace holds a full block of lanes: every check runs at most 64 items
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The run's stream.  Of the LOWEST priority: the runtime keeps a pool of hardware queues per priority, so this stream takes its queue from a pool nothing else of the
// library uses and leaves the mapping of every other stream of the process onto the normal pool's few queues (GPU_MAX_HW_QUEUES) exactly as it would be without the
// self-test -- a stream of the normal priority, created and destroyed here, moved later streams to other queues, and the two sub-batch streams of a Groth16 batch
// met on one (bn254_groth16_stream_overlap).  A health check also has no business competing with another thread's batch.
class OwnStream {
 public:
  OwnStream() = default;
  OwnStream(const OwnStream&) = delete; OwnStream& operator=(const OwnStream&) = delete;
  ~OwnStream() { if (s_) (void)hipStreamDestroy(s_); }
  int ensure() {
    int least = 0, greatest = 0;
    HIPCK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCK(hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, least));
    return BN254_OK;
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

struct Run {
  hipStream_t s = nullptr;
  uint8_t* din = nullptr; uint8_t* dout = nullptr;      // the device copies of the inputs / the outputs, check k at in_off[k] / out_off[k]
  size_t in_off[CK_COUNT], out_off[CK_COUNT];
  int32_t* ws = nullptr; uint8_t* st = nullptr;         // workspace and status bytes of the check that runs
  const int32_t *k0 = nullptr, *gtab = nullptr, *dtab = nullptr, *target = nullptr, *one = nullptr, *msm = nullptr;      // the key on the device
  const uint8_t* in(int k) const { return din + in_off[k]; }
  uint8_t* out(int k) const { return dout + out_off[k]; }
  hipError_t clear_ws() const { return hipMemsetAsync(ws, 0, WS_PROOFS * (size_t)G16_WS_BYTES_PER_PROOF, s); }
};

hipError_t check_fp(const Run& r) {
  const uint8_t* a = r.in(CK_FP);
  return bn254_launch_dbg_fp_mul(a, a + FP_N * 32, r.out(CK_FP), FP_N, r.s);
}
hipError_t check_fp12_lane(const Run& r) {
  const uint8_t *a = r.in(CK_FP12_LANE), *b = a + F12L_N * 384, *c = b + F12L_N * 384;
  hipError_t e = hipSuccess;
  for (int op = 0; op < F12L_OPS && e == hipSuccess; op++)      // op 5 squares a cyclotomic element as it is; op 3 takes any value through the easy part first
    e = bn254_launch_dbg_fp12_op_fmt(op, op == 5 ? c : a, b, r.out(CK_FP12_LANE) + (size_t)op * F12L_N * 384, F12L_N, r.ws, r.st, 0, 0, r.s);
  return e;
}
hipError_t check_fp12_coop(const Run& r) {
  const uint8_t *a = r.in(CK_FP12_COOP), *b = a + F12C_N * 384, *c = b + F12C_N * 384;
  hipError_t e = hipSuccess;
  for (int k = 0; k < F12C_OPS && e == hipSuccess; k++) {
    const CoopOp& o = F12C_OP[k];
    e = r.clear_ws();                                           // VE_S1 of the one-operand operations: zeros, not the last operation's words
    if (e == hipSuccess) e = bn254_launch_dbg_load(r.ws, F12C_N, r.st, (int)VE_F, o.src == 2 ? c : a, 0, r.s);
    if (e == hipSuccess && o.two) e = bn254_launch_dbg_load(r.ws, F12C_N, r.st, (int)VE_S1, b, 0, r.s);
    if (e == hipSuccess) e = bn254_coop12_dbg_op(r.ws, r.st, F12C_N, o.op, o.arg, nullptr, r.s);
    if (e == hipSuccess) e = bn254_launch_dbg_store(r.ws, F12C_N, (int)VE_S0, r.out(CK_FP12_COOP) + (size_t)k * F12C_N * 384, 0, r.s);
  }
  return e;
}
hipError_t check_pairing_lane(const Run& r) {
  const uint8_t* g1 = r.in(CK_PAIRING_LANE);
  return bn254_launch_dbg_pairing(g1, g1 + PAIR_N * 64, r.out(CK_PAIRING_LANE), PAIR_N, r.ws, r.st, r.s);
}
// the exact Groth16 pipeline on the built-in key: the lane form (part_of_larger: never cooperative, whatever the knobs say), or k_g16_prepare and the cooperative kernel
hipError_t check_g16(const Run& r, int k) {
  const uint8_t* in = r.in(k);
  G16LaunchArgs a;
  a.proofs = in + VK_LEN; a.stride = 256; a.inputs = in + VK_LEN + G16_N * 256; a.n_public = 2; a.n = G16_N; a.ws = r.ws; a.status = r.out(k);
  a.msm_tab = r.msm; a.k0 = r.k0; a.gtab = r.gtab; a.dtab = r.dtab; a.target = r.target; a.inputs_match_key = 1; a.key_inputs = 2; a.msm_part = nullptr;
  a.part_of_larger = k == CK_G16_LANE ? 1 : 0;
  hipError_t e = r.clear_ws();
  if (e != hipSuccess) return e;
  return k == CK_G16_LANE ? bn254_launch_g16(a, r.s, nullptr, nullptr) : bn254_launch_dbg_coop12_g16(a, r.s);
}
// the two-pair check on the key's line tables: the points into the workspace as the PlonK path leaves them, the identity flags into the status bytes
hipError_t check_pair2(const Run& r, int k, const uint8_t* d_flags_st) {
  const uint8_t* p0 = r.in(k) + 128 + 128 + 384;
  hipError_t e = r.clear_ws();
  if (e == hipSuccess) e = bn254_launch_dbg_load(r.ws, P2_N, r.st, (int)VE_LX, p0, 4, r.s);
  if (e == hipSuccess) e = bn254_launch_dbg_load(r.ws, P2_N, r.st, (int)VE_CX, p0 + P2_N * 64, 4, r.s);
  if (e == hipSuccess) e = hipMemcpyAsync(r.st, d_flags_st, P2_N, hipMemcpyDeviceToDevice, r.s);      // after the loads: they set PENDING alone
  if (e == hipSuccess)
    e = k == CK_PAIR2_LANE ? bn254_launch_pairing2_fixed_lanes(r.ws, r.st, P2_N, r.gtab, r.dtab, r.one, P2_REJECT, r.s, nullptr, nullptr, nullptr)
                           : bn254_coop12_miller_fixed(r.ws, r.st, P2_N, 2, r.gtab, r.dtab, r.one, P2_REJECT, r.s);
  if (e == hipSuccess) e = hipMemcpyAsync(r.out(k), r.st, P2_N, hipMemcpyDeviceToDevice, r.s);
  return e;
}
hipError_t check_codec(const Run& r) {
  return bn254_launch_g16_decompress(r.in(CK_CODEC), 128, CODEC_N, r.out(CK_CODEC), r.out(CK_CODEC) + CODEC_N * 256, r.s);
}
hipError_t check_sha256(const Run& r, uint64_t pv_bytes) {
  const uint8_t* in = r.in(CK_SHA256);
  const uint64_t* off = (const uint64_t*)(in + SHA_N * 32);
  return bn254_launch_sp1_public_inputs(in, 32, in + SHA_N * 32 + (SHA_N + 1) * 8 + 8, pv_bytes, 0, off, SHA_N, r.out(CK_SHA256), r.out(CK_SHA256) + SHA_N * 64, r.s);
}
}  // namespace

int bn254_selftest_device(int device, const std::vector<uint8_t> in[CK_COUNT], const HostSide& host, std::vector<uint8_t> got[CK_COUNT], float gpu_ms[MS_COUNT]) {
  (void)device;
  int rc;
  for (int k = 0; k < CK_COUNT; k++) if (in[k].size() != in_bytes(k)) return set_err(BN254_E_BAD_ARG, "self-test input of the wrong size");
  Run r;
  size_t in_total = 0, out_total = 0;
  for (int k = 0; k < CK_COUNT; k++) { r.in_off[k] = in_total; in_total += up256(in_bytes(k)); r.out_off[k] = out_total; out_total += up256(out_bytes(k)); }
  const size_t flags_off = in_total;                    // the status bytes of the two-pair checks (PENDING | identity flags), one set per check
  in_total += 2 * up256(P2_N);
  // everything below is released when this function returns, whichever way (the owners' destructors); the guard drains the stream first
  OwnStream stream; Event ev[MS_COUNT + 1];
  PinBuf<uint8_t> h_in, h_out, h_key;
  DevBuf<uint8_t> d_in, d_out, d_st;
  DevBuf<int32_t> d_ws, d_key, d_tab, d_tplane, d_taff, d_plane;
  if ((rc = stream.ensure())) return rc;
  for (auto& e : ev) if ((rc = e.ensure_timed())) return rc;
  if ((rc = h_in.ensure(in_total)) || (rc = h_out.ensure(out_total)) || (rc = d_in.ensure(in_total)) || (rc = d_out.ensure(out_total)) || (rc = d_st.ensure(WS_PROOFS)) ||
      (rc = d_ws.ensure(WS_PROOFS * (size_t)(G16_WS_BYTES_PER_PROOF / 4))))
    return rc;
  HIPCK(bn254_coop12_prepare());                        // the step-kind table of the cooperative kernels, if this device has none yet
  r.s = stream; r.din = d_in; r.dout = d_out; r.ws = d_ws; r.st = d_st;
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{stream};      // declared last: runs before any buffer goes
  memset(h_in, 0, in_total);
  for (int k = 0; k < CK_COUNT; k++) memcpy(h_in + r.in_off[k], in[k].data(), in[k].size());
  for (int q = 0; q < 2; q++) {
    const uint8_t* fl = in[CK_PAIR2_LANE + q].data() + 128 + 128 + 384 + P2_N * 128;
    for (int i = 0; i < P2_N; i++) h_in[flags_off + q * up256(P2_N) + i] = (uint8_t)(BN254_ST_PENDING | ((fl[i] & 1) ? BN254_ST_LINF : 0) | ((fl[i] & 2) ? BN254_ST_LINF2 : 0));
  }
  uint64_t pv_bytes = 0;
  memcpy(&pv_bytes, in[CK_SHA256].data() + SHA_N * 32 + (SHA_N + 1) * 8, 8);
  if (pv_bytes > SHA_PV_BYTES) return set_err(BN254_E_BAD_ARG, "self-test input: the values' buffer is smaller than it says");
  auto launched = [](hipError_t e, int k) { return launch_err(e, bn254_selftest_check_name(k)); };
  hipError_t e;
  HIPCK(hipMemcpyAsync(d_in, h_in, in_total, hipMemcpyHostToDevice, stream));
  HIPCK(hipMemsetAsync(d_out, 0xEE, out_total, stream));
  // the checks that need no key first: the host prepares the key while they run
  int at = 0, order[MS_COUNT];                          // order[j]: what ran between events j and j + 1
  auto mark = [&](int what) -> int { order[at] = what; HIPCK(hipEventRecord(ev[++at], stream)); return BN254_OK; };
  HIPCK(hipEventRecord(ev[0], stream));
  if ((e = check_fp(r)) != hipSuccess) return launched(e, CK_FP);
  if ((rc = mark(CK_FP))) return rc;
  if ((e = check_fp12_lane(r)) != hipSuccess) return launched(e, CK_FP12_LANE);
  if ((rc = mark(CK_FP12_LANE))) return rc;
  if ((e = check_fp12_coop(r)) != hipSuccess) return launched(e, CK_FP12_COOP);
  if ((rc = mark(CK_FP12_COOP))) return rc;
  if ((e = check_pairing_lane(r)) != hipSuccess) return launched(e, CK_PAIRING_LANE);
  if ((rc = mark(CK_PAIRING_LANE))) return rc;
  if ((e = check_codec(r)) != hipSuccess) return launched(e, CK_CODEC);
  if ((rc = mark(CK_CODEC))) return rc;
  if ((e = check_sha256(r, pv_bytes)) != hipSuccess) return launched(e, CK_SHA256);
  if ((rc = mark(CK_SHA256))) return rc;
  // the key: its digits in one block, its window tables built here as ensure_dev builds them (bn254_k_comb.hip, form 2), on this stream
  const Key* key = host.key();
  if (!key) return BN254_E_VK;
  const size_t lines = (size_t)BN_ATE_STEPS * FIXED_LINE_DWORDS, np = 2;
  if (key->k0.size() != 2 * BN_NL || key->gtab.size() != lines || key->dtab.size() != lines || key->target.size() != 12 * BN_NL || key->one.size() != 12 * BN_NL ||
      key->kpts.size() != np * 2 * BN_NL)
    return set_err(BN254_E_BAD_ARG, "self-test key of the wrong shape");
  const size_t key_dwords = 2 * BN_NL + 2 * lines + 2 * 12 * BN_NL + np * 2 * BN_NL;
  const size_t per_point = bn254_tab_build_out_entries(2) * MSM_ENTRY_DWORDS, teeth = bn254_tab_build_teeth(2), entries = bn254_tab_build_entries(2);
  if ((rc = h_key.ensure(key_dwords * 4)) || (rc = d_key.ensure(key_dwords)) || (rc = d_tab.ensure(np * per_point)) || (rc = d_tplane.ensure(np * teeth * 27)) ||
      (rc = d_taff.ensure(np * teeth * 2 * BN_NL)) || (rc = d_plane.ensure(np * entries * 27)))
    return rc;
  {
    int32_t* p = (int32_t*)(uint8_t*)h_key;
    size_t o = 0;
    auto put = [&](const std::vector<int32_t>& v, const int32_t** dev) { memcpy(p + o, v.data(), v.size() * 4); *dev = d_key + o; o += v.size(); };
    const int32_t* kp;
    put(key->k0, &r.k0); put(key->gtab, &r.gtab); put(key->dtab, &r.dtab); put(key->target, &r.target); put(key->one, &r.one); put(key->kpts, &kp);
    HIPCK(hipMemcpyAsync(d_key, h_key, key_dwords * 4, hipMemcpyHostToDevice, stream));
    if ((e = bn254_launch_tab_build(2, kp, (uint32_t)np, d_tab, d_tplane, d_taff, d_plane, stream)) != hipSuccess) return launch_err(e, "self-test key tables");
    r.msm = d_tab;
  }
  if ((rc = mark(MS_KEY))) return rc;
  if ((e = check_g16(r, CK_G16_LANE)) != hipSuccess) return launched(e, CK_G16_LANE);
  if ((rc = mark(CK_G16_LANE))) return rc;
  if ((e = check_g16(r, CK_G16_COOP)) != hipSuccess) return launched(e, CK_G16_COOP);
  if ((rc = mark(CK_G16_COOP))) return rc;
  if ((e = check_pair2(r, CK_PAIR2_LANE, d_in + flags_off)) != hipSuccess) return launched(e, CK_PAIR2_LANE);
  if ((rc = mark(CK_PAIR2_LANE))) return rc;
  if ((e = check_pair2(r, CK_PAIR2_COOP, d_in + flags_off + up256(P2_N))) != hipSuccess) return launched(e, CK_PAIR2_COOP);
  if ((rc = mark(CK_PAIR2_COOP))) return rc;
  HIPCK(hipMemcpyAsync(h_out, d_out, out_total, hipMemcpyDeviceToHost, stream));
  host.overlap();
  HIPCK(hipStreamSynchronize(stream));
  for (int k = 0; k < CK_COUNT; k++) got[k].assign(h_out + r.out_off[k], h_out + r.out_off[k] + out_bytes(k));
  for (int j = 0; j < at; j++) { float ms = 0.f; HIPCK(hipEventElapsedTime(&ms, ev[j], ev[j + 1])); gpu_ms[order[j]] = ms; }
  return BN254_OK;
}
