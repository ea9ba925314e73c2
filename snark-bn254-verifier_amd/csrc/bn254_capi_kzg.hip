// bn254_capi_kzg.hip -- batch verification of KZG openings (include/bn254_verify.h: bn254_kzg_key_prepare, bn254_kzg_verify_batch, _device, bn254_kzg_reserve, the
// knob and the counters bn254_set_kzg_params, bn254_kzg_params, bn254_kzg_state) and what the probe bn254_dbg_kzg_fold (bn254_capi_dbg.hip) runs: kzg_host_call with the probe's buffers, kzg_fold_on_host.
// No handle: the key is plain data.  The launches run on the per-DEVICE pairing workspace of bn254_capi_pairing.hip under its lock and behind its completion event, so
// a KZG call and a pairing call on one device serialise; the term records, rows, window-table scratch and group buffers of the G1 walk are a device's own, grown under
// the same lock.  Launch sequence of one pass of m openings (bn254_kzg.h):
//   exact      k_kzg_load -> k_g1_msm_rows -> k_g1_sum_affine (F to vp_p(0)) -> k_kzg_ident -> the pairing batch behind its load step (mask 0b11, the key's records)
//   weighted   k_kzg_load (weights) -> k_g1_msm_rows -> k_g1_sum_affine (F', H') -> k_plonk_group_sums -> k_kzg_ident on the openings and on the groups -> the pairing
//              batch on the m / 64 groups -> k_plonk_group_scatter -> ONE synchronisation (which groups failed) -> the pairing batch on the openings still pending
// Like bn254_capi_pairing.hip not part of the one-translation-unit host build of bn254_capi.hip: tests/hostsan/hostsan_kzg.cpp includes it itself.
#include "bn254_capi_internal.h"
#include "bn254_capi_pairing.h"
#include "bn254_kzg.h"
#include "bn254_capi_kzg.h"

static_assert(BN254_KZG_OPENING_LEN == KZG_OPENING_LEN, "an opening is six fields of 32 bytes");
static_assert(BN254_KZG_KEY_LEN == KZG_KEY_LEN && KZG_KEY_LEN == 16 + 2 * sizeof(bn254::Fp::v) + 2 * BN254_G2_PREPARED_LEN && sizeof(bn254::Fp::v) == 36,
              "BN254_KZG_KEY_LEN is the header of four dwords, the digits of g1's two Fp and two prepared G2 records");
static_assert(KZG_KEY_REC0_DWORD * 4 % 8 == 0, "the records inside a key keep the key's alignment");
static_assert(BN254_KZG_FOLD_MAX_DIGESTS == KZG_FOLD_MAX_DIGESTS && BN254_KZG_FOLD_MAX_DATA == KZG_FOLD_MAX_DATA && BN254_KZG_FOLD_LEN(1, 0) == BN254_KZG_OPENING_LEN &&
              BN254_KZG_FOLD_LEN(KZG_FOLD_MAX_DIGESTS, KZG_FOLD_MAX_DATA) == KZG_FOLD_LEN(KZG_FOLD_MAX_DIGESTS, KZG_FOLD_MAX_DATA), "the header's limits and record length are the loader's");

size_t KzgForm::rec_len() const { return k ? KZG_FOLD_LEN(k, data_len) : (size_t)KZG_OPENING_LEN; }
int KzgForm::n_terms(bool weighted) const { return k ? KZG_FOLD_TERMS(k, weighted) : weighted ? KZG_TERMS_RLC : KZG_TERMS_EXACT; }
int KzgForm::n_var(bool weighted) const { return k ? k + (weighted ? 3 : 1) : weighted ? 4 : 2; }
size_t KzgForm::max_launch() const { return k ? bn254::kzg_fold_max_launch((size_t)k) : KZG_MAX_LAUNCH; }
static MsmShape kzg_form_shape(const KzgForm& f, bool weighted) { return f.k ? bn254::kzg_fold_msm_shape(f.k, weighted) : bn254::kzg_msm_shape(weighted); }

// the host entries stage a pass through pinned memory of at most this many bytes: the key, then the openings packed
#define KZG_STAGE_BYTES ((size_t)48 << 20)

// BN254_FLAG_RLC is honoured from this many openings per launch on (bn254_set_kzg_params; BN254_KZG_RLC_MIN gives the initial value, read with the launch knobs of
// bn254_g16_plan.h).  The default is what tools/bench_kzg.py measured (profiles/r17_kzg_batch.txt)
static long kzg_rlc_clamp(long v) { return v < (long)KZG_RLC_MIN_FLOOR ? (long)KZG_RLC_MIN_FLOOR : v; }
static std::atomic<long> g_kzg_rlc_min{[] { const long v = bn254::knob_kzg_rlc_min(); return v < 0 ? (long)KZG_RLC_MIN_DEFAULT : kzg_rlc_clamp(v); }()};
// bn254_kzg_state
static std::atomic<uint64_t> g_kzg_state[4];

namespace {

// what a device holds for the G1 walk beside the pairing workspace; guarded by the PbDev's lock
struct KzgDev {
  DevBuf<int32_t> terms, part, glv, grp_ws; DevBuf<uint8_t> flags, st, grp_st;
  size_t part_points = 0, glv_lanes = 0;
  DevBuf<uint32_t> d_fail; PinBuf<uint32_t> h_fail;
  DevBuf<uint8_t> d_out; PinBuf<uint8_t> h_out;   // host entries: the status bytes of a pass on both sides
};
KzgDev* kzg_dev(int device) {      // never destroyed, map nodes never move (pb_dev)
  static std::mutex mu;
  static std::map<int, KzgDev>* devs = new std::map<int, KzgDev>();
  std::lock_guard<std::mutex> lk(mu);
  return &(*devs)[device];
}
inline size_t kzg_pad4(size_t n) { return (n + 3) & ~(size_t)3; }
// caller holds d.mu.  The device ready (self-test at its first use), the pairing workspace and the walk's buffers grown to what launches of up to min(n, the
// workspace's items, KZG_MAX_LAUNCH) openings need; *launch: that many.  weighted: the larger records, rows and scratch of the weighted form and the group buffers
int kzg_ensure(PbDev& d, KzgDev& k, int device, size_t n, bool weighted, size_t* launch, const KzgForm& form = KzgForm()) {
  const size_t max_launch = form.max_launch();
  int rc = pb_ensure(d, device, n < max_launch ? n : max_launch);
  if (rc) return rc;
  size_t cap = d.ws_items() < max_launch ? d.ws_items() : max_launch;
  const size_t need = n < cap ? n : cap;
  *launch = need;
  const int n_terms = form.n_terms(weighted);
  const MsmShape sh = kzg_form_shape(form, weighted);
  const size_t lanes = plonk_scratch_lanes(need, form.n_var(weighted)), points = plonk_part_points(need, sh);
  if ((rc = k.terms.ensure(need * (size_t)n_terms * MSM_TERM_DWORDS)) || (rc = k.flags.ensure(need * (size_t)n_terms)) || (rc = k.st.ensure(kzg_pad4(need)))) return rc;
  if (points > k.part_points) { k.part_points = 0; if ((rc = k.part.ensure(points * 27))) return rc; k.part_points = points; }
  if (lanes > k.glv_lanes) { k.glv_lanes = 0; if ((rc = k.glv.ensure(lanes * (size_t)(G1_GLV_TAB_BYTES_PER_LANE / 4)))) return rc; k.glv_lanes = lanes; }
  if (weighted) {
    const size_t groups = (need + 63) / 64;
    if ((rc = k.grp_ws.ensure(groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = k.grp_st.ensure(kzg_pad4(groups))) || (rc = k.d_fail.ensure(1)) || (rc = k.h_fail.ensure(1))) return rc;
  }
  return BN254_OK;
}

int kzg_pairing(PbDev& d, int32_t* ws, uint8_t* st, size_t n, const int32_t* d_key, int force, hipStream_t s) {
  bn254::PairingLaunchArgs a;
  a.pairs = nullptr; a.item_stride = 0; a.n_pairs = 2; a.n = n; a.ws = ws; a.status = st; a.one = (const int32_t*)d.one; a.out_gt = nullptr;
  a.form = force != bn254::PAIRING_FORM_PLAN ? force : pb_form(2, n);
  if (a.form == bn254::PAIRING_FORM_COOP && n > (size_t)COOP12_MAX_PROOFS) a.form = bn254::PAIRING_FORM_LANES;
  a.shared_mask = 3u; a.prepared = d_key + KZG_KEY_REC0_DWORD; a.skip_load = true;
  const hipError_t e = bn254_launch_pairing_batch(a, s);
  if (e != hipSuccess) return launch_err(e, "KZG pairing check");
  pb_count_launch(a.form);
  return BN254_OK;
}

// One launch of m openings, everything on s; caller holds d.mu and has run kzg_ensure.  d_status: m bytes of the caller's (any alignment).  weighted: the joint check
// (d_weights: the probe's weights, else the ChaCha20 stream of wkey), which synchronises s once.  pr: the probe's device buffers or null
int kzg_launch(PbDev& d, KzgDev& k, const int32_t* d_key, const uint8_t* d_open, size_t stride, size_t m, uint8_t* d_status, bool strict, bool weighted, const uint32_t* d_weights,
               const bn254::ChaChaKey& wkey, int force, hipStream_t s, const KzgProbeDev* pr, const KzgForm& form) {
  const size_t m_pad = (m + 63) & ~(size_t)63, groups = m_pad / 64;
  const int n_terms = form.n_terms(weighted);
  MsmPlan plan;
  if (!msm_plan_build(plan, kzg_form_shape(form, weighted), m_pad, msm_lane_budget(), 0, plonk_joint_g(m_pad))) return set_err(BN254_E_HIP, "KZG: the G1 walk needs more rows than a launch has");
  if (m > d.ws_items() || m > form.max_launch() || bn254_g1_msm_scratch_lanes(plan, m) > k.glv_lanes || (size_t)plan.n_rows * m > k.part_points ||
      k.terms.cap() < m * (size_t)n_terms * MSM_TERM_DWORDS || k.flags.cap() < m * (size_t)n_terms || k.st.cap() < kzg_pad4(m) ||
      (weighted && (k.grp_ws.cap() < groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4) || k.grp_st.cap() < kzg_pad4(groups))))
    return set_err(BN254_E_HIP, "KZG buffers smaller than the launch (internal sizing error)");
  bn254::KzgLoadArgs a;
  a.key = d_key; a.openings = d_open; a.stride = stride; a.n = m; a.ws = d.ws; a.status = k.st; a.terms = k.terms; a.flags = k.flags; a.strict = strict; a.weighted = weighted;
  a.weights = d_weights; a.wkey = wkey;
  a.n_digests = form.k; a.data_len = form.data_len; a.dbg = pr ? pr->fold : nullptr;
  hipError_t e = bn254_launch_kzg_load(a, s);
  // no fixed-base term: the table pointer is never read (any device address)
  if (e == hipSuccess) e = bn254_launch_g1_msm_rows(plan, k.terms, k.flags, m, n_terms, k.part, k.glv, d_key, s);
  if (e == hipSuccess) e = bn254_launch_g1_sum_rows(plan, k.part, m, nullptr, nullptr, d.ws, k.st, bn254::vp_p(0), KZG_ST_F_INF, bn254::vp_p(1), KZG_ST_H_INF, s);
  if (e == hipSuccess && weighted) e = bn254_launch_plonk_group_sums(d.ws, k.st, m, k.grp_ws, k.grp_st, bn254::vp_p(0), KZG_ST_F_INF, bn254::vp_p(1), KZG_ST_H_INF, s);
  if (e == hipSuccess) e = bn254_launch_kzg_ident(d_key, d.ws, k.st, m, s);
  if (e == hipSuccess && pr) e = bn254_launch_kzg_fetch(d.ws, k.st, m, pr->f, pr->h, pr->inf, s);
  if (e != hipSuccess) return launch_err(e, "KZG fold");
  int rc;
  if (!weighted) {
    if ((rc = kzg_pairing(d, d.ws, k.st, m, d_key, force, s))) return rc;
    g_kzg_state[3].fetch_add(1, std::memory_order_relaxed);
  } else {
    e = bn254_launch_kzg_ident(d_key, k.grp_ws, k.grp_st, groups, s);
    if (e == hipSuccess && pr && pr->grp_f) e = bn254_launch_kzg_fetch(k.grp_ws, k.grp_st, groups, pr->grp_f, pr->grp_h, pr->grp_inf, s);
    if (e != hipSuccess) return launch_err(e, "KZG groups");
    if ((rc = kzg_pairing(d, k.grp_ws, k.grp_st, groups, d_key, force, s))) return rc;
    if (pr && pr->grp_st) HIPCK(hipMemcpyAsync(pr->grp_st, k.grp_st, groups, hipMemcpyDeviceToDevice, s));
    HIPCK(hipMemsetAsync(k.d_fail, 0, sizeof(uint32_t), s));
    e = bn254_launch_plonk_group_scatter(k.st, m, k.grp_st, k.d_fail, s);
    if (e != hipSuccess) return launch_err(e, "KZG group scatter");
    HIPCK(hipMemcpyAsync(k.h_fail, k.d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    const uint32_t failed = *(const uint32_t*)k.h_fail;
    g_kzg_state[0].fetch_add(1, std::memory_order_relaxed); g_kzg_state[1].fetch_add(groups, std::memory_order_relaxed); g_kzg_state[2].fetch_add(failed, std::memory_order_relaxed);
    // the openings of a failed group are still pending, on their weighted points: the per-opening check runs on exactly those wavefronts (every kernel of the pairing
    // batch leaves a wavefront without a pending item at once)
    if (failed && (rc = kzg_pairing(d, d.ws, k.st, m, d_key, force, s))) return rc;
  }
  HIPCK(hipMemcpyAsync(d_status, k.st, m, hipMemcpyDeviceToDevice, s));
  return BN254_OK;
}

int kzg_fresh_key(bn254::ChaChaKey& key) {
  uint32_t wkey_words[11];
  for (size_t got = 0; got < sizeof wkey_words;) {
    const ssize_t q = getrandom((uint8_t*)wkey_words + got, sizeof wkey_words - got, 0);
    if (q <= 0) return set_err(BN254_E_HIP, "getrandom failed: no weights for the KZG batch");
    got += (size_t)q;
  }
  for (int i = 0; i < 8; i++) key.k[i] = wkey_words[i];
  for (int i = 0; i < 3; i++) key.nonce[i] = wkey_words[8 + i];
  return BN254_OK;
}

// the launches of a call on device memory: caller holds d.mu; launches of weighted_from openings or more take the weighted form (SIZE_MAX: none; kzg_ensure was told).
// The weights of launch j come from the call's key with the launch number in a nonce word
int kzg_enqueue(PbDev& d, KzgDev& k, const int32_t* d_key, const uint8_t* d_open, size_t stride, size_t n, uint8_t* d_status, unsigned flags, size_t launch, int force, hipStream_t s,
                size_t weighted_from, const uint32_t* d_weights = nullptr, const KzgProbeDev* pr = nullptr, const KzgForm& form = KzgForm()) {
  if (d.busy_valid) HIPCK(hipStreamWaitEvent(s, d.busy_ev, 0));
  bn254::ChaChaKey wkey;
  memset(&wkey, 0, sizeof wkey);
  bool have_key = false;
  int rc = BN254_OK;
  uint32_t pass = 0;
  for (size_t off = 0; off < n && !rc; off += launch, pass++) {
    const size_t m = n - off < launch ? n - off : launch;
    const bool weighted = m >= weighted_from;
    if (weighted && !d_weights && !have_key) { if ((rc = kzg_fresh_key(wkey))) break; have_key = true; }
    bn254::ChaChaKey pk = wkey;
    pk.nonce[2] ^= pass;
    rc = kzg_launch(d, k, d_key, d_open + off * stride, stride, m, d_status + off, (flags & BN254_FLAG_STRICT_SCALARS) != 0, weighted, d_weights ? d_weights + 4 * off : nullptr, pk, force, s, pr, form);
  }
  // also after a failure: whatever was enqueued must be behind the event the next call waits for
  const hipError_t e = hipEventRecord(d.busy_ev, s);
  if (e == hipSuccess) d.busy_valid = true;
  if (!rc && e != hipSuccess) return set_err(BN254_E_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
  return rc;
}

// a probe's weight: 16 big-endian bytes -> four little-endian words, forced odd
void kzg_weight_words(uint32_t w[4], const uint8_t* be16) {
  for (int q = 0; q < 4; q++) { const uint8_t* b = be16 + 4 * (3 - q); w[q] = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | (uint32_t)b[3]; }
  w[0] |= 1u;
}
bool kzg_key_host_ok(const uint8_t* key) {
  uint32_t h[2], r0[2], r1[2];
  memcpy(h, key, sizeof h); memcpy(r0, key + 4 * KZG_KEY_REC0_DWORD, sizeof r0); memcpy(r1, key + 4 * KZG_KEY_REC0_DWORD + PB_PREP_LEN, sizeof r1);
  return h[0] == KZG_KEY_MAGIC && h[1] == KZG_KEY_VERSION && r0[0] == PB_PREP_MAGIC && r0[1] == PB_PREP_VERSION && r1[0] == PB_PREP_MAGIC && r1[1] == PB_PREP_VERSION;
}

}  // namespace

// BN254_E_BAD_ARG before any device is touched; *done: n == 0
int kzg_fold_form(size_t n_digests, size_t data_len, KzgForm* form) {
  if (n_digests < 1 || n_digests > (size_t)KZG_FOLD_MAX_DIGESTS) return set_err(BN254_E_BAD_ARG, "bad argument: n_digests is 1 .. BN254_KZG_FOLD_MAX_DIGESTS");
  if (data_len > (size_t)KZG_FOLD_MAX_DATA) return set_err(BN254_E_BAD_ARG, "bad argument: data_len above BN254_KZG_FOLD_MAX_DATA");
  form->k = (int)n_digests; form->data_len = (int)data_len;
  return BN254_OK;
}
int kzg_check_args(const void* key, const void* openings, size_t stride, size_t n, const void* status, unsigned flags, bool host_key, bool* done, const KzgForm& form) {
  *done = false;
  if (flags & ~(unsigned)(BN254_FLAG_STRICT_SCALARS | BN254_FLAG_RLC)) return set_err(BN254_E_BAD_ARG, "bad argument: flags other than BN254_FLAG_STRICT_SCALARS and BN254_FLAG_RLC");
  if (stride < form.rec_len()) return set_err(BN254_E_BAD_ARG, form.k ? "bad argument: stride below BN254_KZG_FOLD_LEN(n_digests, data_len)" : "bad argument: stride below 192");
  if (n && (!key || !openings || !status)) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n && stride > SIZE_MAX / n) return set_err(BN254_E_BAD_ARG, "bad argument: n openings of stride bytes overflow the address space");
  if (n && host_key && !kzg_key_host_ok((const uint8_t*)key)) return set_err(BN254_E_BAD_ARG, "bad argument: a KZG key with a wrong magic word or layout version (bn254_kzg_key_prepare of this library writes it)");
  if (n && !host_key && ((uintptr_t)key & 3)) return set_err(BN254_E_BAD_ARG, "bad argument: d_key is not 4-byte aligned");
  *done = n == 0;
  return BN254_OK;
}

// a host-buffer call: passes through the pinned staging of the pairing entries (the key in front of every pass's openings, packed); weights: the probe's (n x 16 bytes)
int kzg_host_call(const uint8_t* key, const uint8_t* openings, size_t stride, size_t n, uint8_t* status, int device, unsigned flags, int force, const uint8_t* weights, bool force_weighted,
                  KzgProbeHost* ph, const KzgForm& form) {
  std::vector<uint8_t> unit;
  if (force_weighted && !weights) {      // the probe without weights: all 1, never the ChaCha20 stream
    unit.assign(16 * n, 0);
    for (size_t i = 0; i < n; i++) unit[16 * i + 15] = 1;
    weights = unit.data();
  }
  PbDev* d = pb_dev(device);
  KzgDev* k = kzg_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  // a staged record: padded to whole dwords (the weights behind the records and the loader's dword loads want it)
  const size_t lead = KZG_KEY_LEN, wbytes = weights ? 16 : 0, olen = form.rec_len(), slen = (olen + 3) & ~(size_t)3, rec = slen + wbytes;
  size_t launch = 0;
  int rc;
  // ONE reading of the knob per call (bn254_set_kzg_params may run beside it): what kzg_ensure sizes for is what the launches take
  const size_t rlc_min = (size_t)g_kzg_rlc_min.load(std::memory_order_relaxed);
  const size_t weighted_from = force_weighted ? 0 : ((flags & BN254_FLAG_RLC) && n >= rlc_min) ? rlc_min : SIZE_MAX;
  if ((rc = kzg_ensure(*d, *k, device, n, weighted_from != SIZE_MAX, &launch, form)) || (rc = d->stream.ensure())) return rc;
  size_t pass = (KZG_STAGE_BYTES - lead) / rec;
  if (pass > launch) pass = launch;
  if (ph && n > pass) return set_err(BN254_E_BAD_ARG, "bad argument: the probe takes one pass");
  if ((rc = d->h_in.ensure(lead + pass * rec)) || (rc = d->d_in.ensure(lead + pass * rec)) || (rc = k->h_out.ensure(pass)) || (rc = k->d_out.ensure(pass))) return rc;
  hipStream_t s = d->stream;
  KzgProbeDev pr; DevBuf<uint8_t> probe_buf;
  const size_t groups = (n + 63) / 64;
  if (ph) {
    if ((rc = probe_buf.ensure(130 * n + 131 * groups + (ph->fold ? 64 * n : 0)))) return rc;
    uint8_t* b = probe_buf;
    pr.f = b; pr.h = b + 64 * n; pr.inf = b + 128 * n;
    if (ph->fold) pr.fold = b + 130 * n + 131 * groups;
    b += 130 * n;
    pr.grp_f = pr.grp_h = pr.grp_inf = pr.grp_st = nullptr;
    if (ph->grp) { pr.grp_f = b; pr.grp_h = b + 64 * groups; pr.grp_inf = b + 128 * groups; pr.grp_st = b + 130 * groups; }
  }
  auto one_pass = [&](size_t off, size_t m) -> int {
    memcpy(d->h_in, key, lead);
    uint8_t* o = d->h_in + lead;
    if (stride == olen && olen == slen) parallel_copy(o, openings + off * stride, m * slen);
    else for (size_t i = 0; i < m; i++) memcpy(o + i * slen, openings + (off + i) * stride, olen);
    if (weights)      // as little-endian words behind the openings (a multiple of 4 bytes in)
      for (size_t i = 0; i < m; i++) { uint32_t w4[4]; kzg_weight_words(w4, weights + 16 * (off + i)); memcpy(o + m * slen + 16 * i, w4, 16); }
    HIPCK(hipMemcpyAsync(d->d_in, d->h_in, lead + m * rec, hipMemcpyHostToDevice, s));
    const uint8_t* d_open = d->d_in + lead;
    int r = kzg_enqueue(*d, *k, (const int32_t*)(uint8_t*)d->d_in, d_open, slen, m, k->d_out, flags, launch, force, s,
                        weighted_from, weights ? (const uint32_t*)(d_open + m * slen) : nullptr, ph ? &pr : nullptr, form);
    if (r) return r;
    HIPCK(hipMemcpyAsync(k->h_out, k->d_out, m, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    memcpy(status + off, k->h_out, m);
    if (ph) {
      std::vector<uint8_t> hb(130 * n + 131 * groups + (ph->fold ? 64 * n : 0));
      HIPCK(hipMemcpy(hb.data(), probe_buf, hb.size(), hipMemcpyDeviceToHost));
      if (ph->fold) memcpy(ph->fold, hb.data() + 130 * n + 131 * groups, 64 * n);
      memcpy(ph->f, hb.data(), 64 * n); memcpy(ph->h, hb.data() + 64 * n, 64 * n); memcpy(ph->inf, hb.data() + 128 * n, 2 * n);
      if (ph->grp) {
        const uint8_t* g = hb.data() + 130 * n;
        for (size_t q = 0; q < groups; q++) {
          uint8_t* r131 = ph->grp + 131 * q;
          memcpy(r131, g + 64 * q, 64); memcpy(r131 + 64, g + 64 * groups + 64 * q, 64); memcpy(r131 + 128, g + 128 * groups + 2 * q, 2); r131[130] = g[130 * groups + q];
        }
      }
    }
    return BN254_OK;
  };
  for (size_t off = 0; off < n; off += pass) {
    if ((rc = one_pass(off, n - off < pass ? n - off : pass))) {
      const std::string keep = g_err;      // the staging must be quiescent when the lock is released
      (void)hipStreamSynchronize(s);
      return set_err(rc, keep);
    }
  }
  return BN254_OK;
}

// ---- the host compile: the loader, the rows of the plan, the sums, the group sums and the pairing checks on plain arrays (bn254_dbg_kzg_fold with device -1) -------
namespace {
struct KzgHostIO {      // DevMsmIO on host arrays
  const int32_t* t; const uint8_t* f;
  void term(int q, bn254::G1Aff& P, uint32_t k1[4], uint32_t k2[4], uint32_t& fl) const {
    const int32_t* e = t + (size_t)q * MSM_TERM_DWORDS;
    for (int l = 0; l < BN_NL; l++) { P.x.v[l] = e[l]; P.y.v[l] = e[BN_NL + l]; }
    BN_SETB(P.x, 1.0, 0.5); BN_SETB(P.y, 1.0, 0.5);
    for (int w = 0; w < 4; w++) { k1[w] = (uint32_t)e[18 + w]; k2[w] = (uint32_t)e[22 + w]; }
    fl = f[q];
  }
  uint32_t kword(int q, int half, int w) const { return (uint32_t)t[(size_t)q * MSM_TERM_DWORDS + 18 + 4 * half + w]; }
  uint32_t scalar_digit(int, int) const { return 0; }
  bn254::G1Aff entry(int, int, uint32_t) const { bn254::G1Aff z; z.x = bn254::fp_zero(); z.y = bn254::fp_zero(); return z; }
};
struct KzgHostTab {
  bn254::G1Proj* t;
  void put(int i, const bn254::G1Proj& p) { t[i].x = bn254::fp_reduce(p.x); t[i].y = bn254::fp_reduce(p.y); t[i].z = bn254::fp_reduce(p.z); }
  bn254::G1Proj get(uint32_t i) const { return t[i]; }
  void fence() {}
  KzgHostTab slot(int j) const { return KzgHostTab{t + 16 * j}; }
};
// k_g1_sum_affine for sum s of one item: the rows added up, to affine ((0, 1) and the flag for the identity)
void kzg_host_sum(const MsmPlan& plan, int s, KzgHostIO& io, bn254::PbHostLane& w, uint8_t& st, int e_x, int inf_bit) {
  using namespace bn254;
  std::vector<G1Proj> store(16 * MSM_MAX_JOINT);
  G1Proj L = g1_identity();
  for (int r = plan.first[s]; r < plan.first[s] + plan.count[s]; r++) {
    KzgHostTab tab{store.data()};
    G1Proj row = msm_row_eval(plan, r, io, tab);
    BN_SETB(row.x, 3.0, 0.5); BN_SETB(row.y, 3.0, 0.5); BN_SETB(row.z, 3.0, 0.5);
    L = g1_add(L, row);
  }
  const bool inf = g1_is_identity(L);
  G1Aff a = g1_to_affine(L);
  a.y = fp_select(inf, fp_one(), a.y);
  w.st(e_x, a.x); w.st(e_x + 1, a.y);
  if (inf && (st & BN254_ST_PENDING)) st |= (uint8_t)inf_bit;
}
void kzg_host_fetch(const bn254::PbHostLane& w, uint8_t st, uint8_t* f, uint8_t* h, uint8_t* inf) {
  using namespace bn254;
  const bool pend = (st & BN254_ST_PENDING) != 0;
  const uint32_t ident = pend ? pb_ident(w) : 0u;
  for (int j = 0; j < 2; j++) {
    uint8_t* o = j ? h : f;
    const bool is_inf = ((ident >> (2 * j)) & 1u) != 0;
    inf[j] = is_inf ? 1 : 0;
    memset(o, 0, 64);
    if (!pend || is_inf) continue;
    uint32_t v[8];
    fp_to_words(v, w.ld(vp_p(j))); words_to_be(o, v);
    fp_to_words(v, w.ld(vp_p(j) + 1)); words_to_be(o + 32, v);
  }
}
}  // namespace

int kzg_fold_on_host(const uint8_t* key_bytes, const uint8_t* openings, size_t stride, size_t n, const uint8_t* weights, unsigned flags, bool weighted, KzgProbeHost& ph, uint8_t* status,
                     const KzgForm& form) {
  using namespace bn254;
  std::vector<int32_t> key(KZG_KEY_DWORDS);      // the caller's bytes need not be aligned
  memcpy(key.data(), key_bytes, KZG_KEY_LEN);
  const int n_terms = form.n_terms(weighted);
  const size_t n_pad = (n + 63) & ~(size_t)63, groups = n_pad / 64;
  MsmPlan plan;
  if (!msm_plan_build(plan, kzg_form_shape(form, weighted), n_pad, msm_lane_budget(), 0, plonk_joint_g(n_pad))) return set_err(BN254_E_HIP, "KZG: the G1 walk needs more rows than a launch has");
  const int run_steps = knob_run_steps_pairing_batch();
  const int32_t* recs = key.data() + KZG_KEY_REC0_DWORD;
  std::vector<PbHostLane> ws(n), gws(weighted ? groups : 0);
  std::vector<uint8_t> st(n), gst(groups, 0);
  std::vector<int32_t> terms((size_t)n_terms * MSM_TERM_DWORDS);
  std::vector<uint8_t> fl(n_terms);
  const bool key_ok = kzg_key_header_ok(key.data());
  for (size_t i = 0; i < n; i++) {
    PbHostLane& w = ws[i];
    for (auto& x : w.e) x = fp_zero();
    if (ph.fold) memset(ph.fold + 64 * i, 0, 64);
    if (!key_ok) { st[i] = BN254_ST_MALFORMED; continue; }
    uint32_t wgt[4] = {1, 0, 0, 0};
    if (weights) kzg_weight_words(wgt, weights + 16 * i);
    const bool strict = (flags & BN254_FLAG_STRICT_SCALARS) != 0;
    st[i] = form.k ? (uint8_t)kzg_fold_load_record(w, openings + i * stride, false, form.k, form.data_len, key.data(), strict, weighted ? wgt : nullptr, terms.data(), fl.data(),
                                                   ph.fold ? ph.fold + 64 * i : nullptr)
                   : (uint8_t)kzg_load_opening(w, openings + i * stride, false, key.data(), strict, weighted ? wgt : nullptr, terms.data(), fl.data());
    KzgHostIO io{terms.data(), fl.data()};
    kzg_host_sum(plan, 0, io, w, st[i], vp_p(0), KZG_ST_F_INF);
    if (weighted) kzg_host_sum(plan, 1, io, w, st[i], vp_p(1), KZG_ST_H_INF);
  }
  if (weighted)
    for (size_t g = 0; g < groups; g++) {      // k_plonk_group_sums
      PbHostLane& gw = gws[g];
      for (auto& x : gw.e) x = fp_zero();
      bool any = false;
      uint8_t gflags = 0;
      for (int which = 0; which < 2; which++) {
        G1Proj L = g1_identity();
        for (size_t i = 64 * g; i < 64 * g + 64 && i < n; i++) {
          if (!(st[i] & BN254_ST_PENDING)) continue;
          any = true;
          if (st[i] & (which ? KZG_ST_H_INF : KZG_ST_F_INF)) continue;
          G1Aff p; p.x = ws[i].ld(vp_p(which)); p.y = ws[i].ld(vp_p(which) + 1);
          L = g1_add(L, g1_from_affine(p));
        }
        const bool inf = g1_is_identity(L);
        G1Aff a = g1_to_affine(L);
        a.y = fp_select(inf, fp_one(), a.y);
        gw.st(vp_p(which), a.x); gw.st(vp_p(which) + 1, a.y);
        if (inf) gflags |= (uint8_t)(which ? KZG_ST_H_INF : KZG_ST_F_INF);
      }
      gst[g] = any ? (uint8_t)(BN254_ST_PENDING | gflags) : (uint8_t)BN254_ST_ACCEPT;
    }
  for (size_t i = 0; i < n; i++) {
    if (st[i] & BN254_ST_PENDING) { kzg_finish_item(ws[i], key.data(), st[i]); st[i] = BN254_ST_PENDING; }
    kzg_host_fetch(ws[i], st[i], ph.f + 64 * i, ph.h + 64 * i, ph.inf + 2 * i);
  }
  if (weighted) {
    for (size_t g = 0; g < groups; g++) {
      if (gst[g] & BN254_ST_PENDING) { kzg_finish_item(gws[g], key.data(), gst[g]); gst[g] = BN254_ST_PENDING; }
      uint8_t* r131 = ph.grp ? ph.grp + 131 * g : nullptr;
      if (r131) kzg_host_fetch(gws[g], gst[g], r131, r131 + 64, r131 + 128);
      if (gst[g] & BN254_ST_PENDING) gst[g] = pb_lane_shared_on_host(gws[g], 2, 3u, recs, nullptr, run_steps);
      if (r131) r131[130] = gst[g];
    }
    for (size_t i = 0; i < n; i++) if ((st[i] & BN254_ST_PENDING) && gst[i / 64] == BN254_ST_ACCEPT) st[i] = BN254_ST_ACCEPT;      // k_plonk_group_scatter
  }
  for (size_t i = 0; i < n; i++) {
    if (st[i] & BN254_ST_PENDING) st[i] = pb_lane_shared_on_host(ws[i], 2, 3u, recs, nullptr, run_steps);
    status[i] = st[i];
  }
  return BN254_OK;
}

extern "C" {

int bn254_kzg_key_prepare(const uint8_t g1[64], const uint8_t g2[128], const uint8_t tau_g2[128], uint8_t out[BN254_KZG_KEY_LEN], uint8_t* status) {
  if (!g1 || !g2 || !tau_g2 || !out || !status) return set_err(BN254_E_BAD_ARG, "bad argument");
  bool memb = true, zero = true;
  bn254::G1Aff p;
  p.x = bn254::pb_field(g1, false, memb, zero); p.y = bn254::pb_field(g1 + 32, false, memb, zero);
  if (!memb) { *status = BN254_ERR_NOT_MEMBER; return BN254_OK; }
  if (!zero && !bn254::g1_on_curve(p)) { *status = BN254_ERR_NOT_ON_CURVE; return BN254_OK; }
  std::vector<uint8_t> rec(KZG_KEY_LEN, 0);
  const uint32_t hdr[4] = {KZG_KEY_MAGIC, KZG_KEY_VERSION, zero ? KZG_KEY_FLAG_G1_IDENTITY : 0u, 0u};
  memcpy(rec.data(), hdr, sizeof hdr);
  memcpy(rec.data() + 16, p.x.v, sizeof p.x.v); memcpy(rec.data() + 16 + sizeof p.x.v, p.y.v, sizeof p.y.v);
  for (int j = 0; j < 2; j++) {
    uint8_t st = BN254_ERR_MALFORMED;
    const int rc = bn254_g2_prepare(j ? tau_g2 : g2, rec.data() + 4 * KZG_KEY_REC0_DWORD + (size_t)j * PB_PREP_LEN, &st);
    if (rc) return rc;
    if (st != BN254_ACCEPT) { *status = st; return BN254_OK; }
  }
  memcpy(out, rec.data(), KZG_KEY_LEN);
  *status = BN254_ACCEPT;
  return BN254_OK;
}

int bn254_kzg_reserve(size_t n, int device) {
  PbDev* d = pb_dev(device);
  KzgDev* k = kzg_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  size_t launch;
  return kzg_ensure(*d, *k, device, n ? n : 1, false, &launch);
}

int bn254_kzg_verify_batch(const uint8_t* key, const uint8_t* openings, size_t stride, size_t n, uint8_t* status, int device, unsigned flags) {
  bool done;
  const int rc = kzg_check_args(key, openings, stride, n, status, flags, true, &done);
  if (rc || done) return rc;
  return kzg_host_call(key, openings, stride, n, status, device, flags, bn254::PAIRING_FORM_PLAN, nullptr, false, nullptr);
}

int bn254_kzg_verify_batch_device(const void* d_key, const void* d_openings, size_t stride, size_t n, void* d_status, int device, void* hip_stream, unsigned flags) {
  bool done;
  int rc = kzg_check_args(d_key, d_openings, stride, n, d_status, flags, false, &done);
  if (rc || done) return rc;
  PbDev* d = pb_dev(device);
  KzgDev* k = kzg_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  // without BN254_FLAG_RLC nothing is allocated when a reservation (or an earlier call) of min(n, 2^18) openings stands; the weighted form grows its own buffers, and
  // synchronises anyway
  const size_t rlc_min = (size_t)g_kzg_rlc_min.load(std::memory_order_relaxed);
  const size_t weighted_from = ((flags & BN254_FLAG_RLC) && n >= rlc_min) ? rlc_min : SIZE_MAX;
  size_t launch;
  if ((rc = kzg_ensure(*d, *k, device, n, weighted_from != SIZE_MAX, &launch))) return rc;
  return kzg_enqueue(*d, *k, (const int32_t*)d_key, (const uint8_t*)d_openings, stride, n, (uint8_t*)d_status, flags, launch, bn254::PAIRING_FORM_PLAN, (hipStream_t)hip_stream,
                     weighted_from);
}

// the batch-opening entries answer BN254_E_NOMEM for memory that runs out, on the device or pinned (the entries on openings keep the code they had; the owners of
// bn254_capi_owners.h name the runtime's error in the message)
static int kzg_fold_rc(int rc) { return rc == BN254_E_HIP && g_err.find("out of memory") != std::string::npos ? set_err(BN254_E_NOMEM, std::string(g_err)) : rc; }

int bn254_kzg_fold_reserve(size_t n, size_t n_digests, int device) {
  KzgForm form;
  const int rc = kzg_fold_form(n_digests, 0, &form);
  if (rc) return rc;
  PbDev* d = pb_dev(device);
  KzgDev* k = kzg_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  size_t launch;
  return kzg_fold_rc(kzg_ensure(*d, *k, device, n ? n : 1, false, &launch, form));
}

int bn254_kzg_verify_folded_batch(const uint8_t* key, const uint8_t* records, size_t stride, size_t n, size_t n_digests, size_t data_len, uint8_t* status, int device, unsigned flags) {
  KzgForm form;
  bool done;
  int rc = kzg_fold_form(n_digests, data_len, &form);
  if (rc || (rc = kzg_check_args(key, records, stride, n, status, flags, true, &done, form)) || done) return rc;
  return kzg_fold_rc(kzg_host_call(key, records, stride, n, status, device, flags, bn254::PAIRING_FORM_PLAN, nullptr, false, nullptr, form));
}

int bn254_kzg_verify_folded_batch_device(const void* d_key, const void* d_records, size_t stride, size_t n, size_t n_digests, size_t data_len, void* d_status, int device, void* hip_stream,
                                         unsigned flags) {
  KzgForm form;
  bool done;
  int rc = kzg_fold_form(n_digests, data_len, &form);
  if (rc || (rc = kzg_check_args(d_key, d_records, stride, n, d_status, flags, false, &done, form)) || done) return rc;
  PbDev* d = pb_dev(device);
  KzgDev* k = kzg_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  // as bn254_kzg_verify_batch_device: without BN254_FLAG_RLC nothing is allocated when a reservation of min(n, a pass) records of n_digests digests stands
  const size_t rlc_min = (size_t)g_kzg_rlc_min.load(std::memory_order_relaxed);
  const size_t weighted_from = ((flags & BN254_FLAG_RLC) && n >= rlc_min) ? rlc_min : SIZE_MAX;
  size_t launch;
  if ((rc = kzg_ensure(*d, *k, device, n, weighted_from != SIZE_MAX, &launch, form))) return kzg_fold_rc(rc);
  return kzg_fold_rc(kzg_enqueue(*d, *k, (const int32_t*)d_key, (const uint8_t*)d_records, stride, n, (uint8_t*)d_status, flags, launch, bn254::PAIRING_FORM_PLAN, (hipStream_t)hip_stream,
                                 weighted_from, nullptr, nullptr, form));
}

void bn254_set_kzg_params(long rlc_min) {
  if (rlc_min >= 0) g_kzg_rlc_min.store(kzg_rlc_clamp(rlc_min));
}
int bn254_kzg_params(long out[1]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  out[0] = g_kzg_rlc_min.load();
  return BN254_OK;
}
int bn254_kzg_state(uint64_t out[4]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  for (int i = 0; i < 4; i++) out[i] = g_kzg_state[i].load(std::memory_order_relaxed);
  return BN254_OK;
}

}  // extern "C"
