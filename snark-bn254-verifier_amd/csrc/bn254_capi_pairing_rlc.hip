// bn254_capi_pairing_rlc.hip -- BN254_FLAG_RLC for the batch pairing product (include/bn254_verify.h: bn254_pairing_check_batch_flags, _device, the knob and the
// counters bn254_set_pairing_rlc_params, bn254_pairing_rlc_params, bn254_pairing_rlc_state) and the probe bn254_dbg_pairing_batch_rlc.  The launches run on the
// per-DEVICE pairing workspace of bn254_capi_pairing.hip under its lock and behind its completion event; the group workspace and the padded status bytes are a
// device's own, grown under the same lock.  Launch sequence of one launch of m items (bn254_pairing_rlc.h):
//   exact      the launch of bn254_pairing_check_batch_shared
//   weighted   the loader -> k_pairing_rlc_weigh -> the Miller runs over the variable positions -> k_pairing_rlc_group_sums, k_pairing_rlc_group_prod -> the check of
//              the m / 64 groups -> k_plonk_group_scatter -> ONE synchronisation (which groups failed) -> the exact launch behind its loader on the items still pending
// Like bn254_capi_pairing.hip not part of the one-translation-unit host build of bn254_capi.hip: tests/hostsan/hostsan_pairing_rlc.cpp includes it itself.
#include "bn254_capi_internal.h"
#include "bn254_capi_pairing.h"
#include "bn254_pairing_rlc.h"
#include "bn254_capi_pairing_rlc.h"

static long pbr_rlc_clamp(long v) { return v < (long)PBR_RLC_MIN_FLOOR ? (long)PBR_RLC_MIN_FLOOR : v; }
static std::atomic<long> g_pbr_rlc_min{[] { const long v = env_long("BN254_PAIRING_RLC_MIN", -1); return v < 0 ? (long)PBR_RLC_MIN_DEFAULT : pbr_rlc_clamp(v); }()};
// the most variable positions of a shape the flag is honoured for (bn254_dbg_set_pairing_rlc_max_var: tests)
static std::atomic<int> g_pbr_max_var{PBR_MAX_VAR_HONOURED};
// bn254_pairing_rlc_state
static std::atomic<uint64_t> g_pbr_state[4];

namespace {

// what a device holds for the joint check beside the pairing workspace; guarded by the PbDev's lock
struct PbrDev {
  DevBuf<int32_t> grp_ws; DevBuf<uint8_t> st, grp_st;
  DevBuf<uint32_t> d_fail; PinBuf<uint32_t> h_fail;
  DevBuf<uint8_t> d_out; PinBuf<uint8_t> h_out;   // host entries: the status bytes of a pass on both sides
};
PbrDev* pbr_dev(int device) {      // never destroyed, map nodes never move (pb_dev)
  static std::mutex mu;
  static std::map<int, PbrDev>* devs = new std::map<int, PbrDev>();
  std::lock_guard<std::mutex> lk(mu);
  return &(*devs)[device];
}
inline size_t pbr_pad4(size_t n) { return (n + 3) & ~(size_t)3; }
// the probe's device buffers of one launch: the GT value and the status of every group, the status bytes as the Miller runs left them, the status bytes and GT values of
// the exact check of every item on its weighted points
struct PbrProbeDev { uint8_t *grp_gt, *grp_st, *st_mid, *st_item, *item_gt; };

// the flag is honoured for a launch of m items of this shape?
bool pbr_honoured(size_t n_pairs, unsigned mask, size_t m, size_t rlc_min) {
  const int n_var = (int)n_pairs - __builtin_popcount(mask);
  return m >= rlc_min && n_var <= g_pbr_max_var.load(std::memory_order_relaxed);
}
// caller holds d.mu: the pairing workspace for launches of min(n, a pass) items and, weighted, the group buffers for them
int pbr_ensure(PbDev& d, PbrDev& k, int device, size_t n, bool weighted) {
  int rc = pb_ensure(d, device, n);
  if (rc || !weighted) return rc;
  const size_t need = pb_ws_items_of(n), groups = (need + 63) / 64;
  if ((rc = k.grp_ws.ensure(groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = k.grp_st.ensure(pbr_pad4(groups))) || (rc = k.st.ensure(pbr_pad4(need))) ||
      (rc = k.d_fail.ensure(1)) || (rc = k.h_fail.ensure(1)))
    return rc;
  return BN254_OK;
}
int pbr_exact(PbDev& d, const uint8_t* d_items, size_t stride, size_t n_pairs, const PbShared& sh, size_t m, int32_t* ws, uint8_t* st, bool skip_load, int force, uint8_t* out_gt,
              hipStream_t s) {
  bn254::PairingLaunchArgs a;
  a.pairs = d_items; a.item_stride = stride; a.n_pairs = (int)n_pairs; a.n = m; a.ws = ws; a.status = st; a.one = (const int32_t*)d.one; a.out_gt = out_gt;
  a.form = force != bn254::PAIRING_FORM_PLAN ? force : pb_form(n_pairs, m);
  if (a.form == bn254::PAIRING_FORM_COOP && m > (size_t)COOP12_MAX_PROOFS) a.form = bn254::PAIRING_FORM_LANES;
  a.shared_mask = sh.mask; a.prepared = (const int32_t*)sh.prepared; a.skip_load = skip_load;
  const hipError_t e = bn254_launch_pairing_batch(a, s);
  if (e != hipSuccess) return launch_err(e, "pairing batch");
  pb_count_launch(a.form);
  return BN254_OK;
}
// One weighted launch of m items, everything on s, ONE synchronisation; caller holds d.mu and has run pbr_ensure.  d_status: m bytes of the caller's (any alignment).
// d_weights: the probe's weights, else the ChaCha20 stream of wkey.  pr: the probe's buffers -- then the launch ends with the exact check of EVERY item that reached
// the groups, in place of the scatter and the fallback (the caller puts the status bytes together)
int pbr_launch(PbDev& d, PbrDev& k, const uint8_t* d_items, size_t stride, size_t n_pairs, const PbShared& sh, size_t m, uint8_t* d_status, const uint32_t* d_weights,
               const bn254::ChaChaKey& wkey, int force, hipStream_t s, const PbrProbeDev* pr) {
  const size_t groups = (m + 63) / 64;
  if (m > d.ws_items() || k.st.cap() < pbr_pad4(m) || k.grp_ws.cap() < groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4) || k.grp_st.cap() < pbr_pad4(groups))
    return set_err(BN254_E_HIP, "pairing RLC buffers smaller than the launch (internal sizing error)");
  bn254::PairingLaunchArgs l;
  l.pairs = d_items; l.item_stride = stride; l.n_pairs = (int)n_pairs; l.n = m; l.ws = d.ws; l.status = k.st; l.one = (const int32_t*)d.one; l.out_gt = nullptr;
  l.form = bn254::PAIRING_FORM_LANES; l.shared_mask = sh.mask; l.prepared = (const int32_t*)sh.prepared; l.load_only = true;
  hipError_t e = bn254_launch_pairing_batch(l, s);
  if (e != hipSuccess) return launch_err(e, "pairing RLC load");
  bn254::PairingRlcArgs a;
  a.n_pairs = (int)n_pairs; a.shared_mask = sh.mask; a.prepared = (const int32_t*)sh.prepared; a.n = m; a.ws = d.ws; a.status = k.st; a.grp_ws = k.grp_ws; a.grp_status = k.grp_st;
  a.weights = d_weights; a.wkey = wkey; a.one = (const int32_t*)d.one;
  const size_t grp_pairs = sh.count() ? sh.count() : 1;
  a.grp_form = force != bn254::PAIRING_FORM_PLAN ? force : pb_form(grp_pairs, groups);
  a.out_grp_gt = pr ? pr->grp_gt : nullptr;
  if ((e = bn254_launch_pairing_rlc_joint(a, s)) != hipSuccess) return launch_err(e, "pairing RLC joint check");
  int rc;
  if (pr) {
    HIPCK(hipMemcpyAsync(pr->grp_st, k.grp_st, groups, hipMemcpyDeviceToDevice, s));
    HIPCK(hipMemcpyAsync(pr->st_mid, k.st, m, hipMemcpyDeviceToDevice, s));
    HIPCK(hipMemcpyAsync(pr->st_item, k.st, m, hipMemcpyDeviceToDevice, s));
    if ((rc = pbr_exact(d, nullptr, 0, n_pairs, sh, m, d.ws, pr->st_item, true, force, pr->item_gt, s))) return rc;
    HIPCK(hipStreamSynchronize(s));
    return BN254_OK;
  }
  HIPCK(hipMemsetAsync(k.d_fail, 0, sizeof(uint32_t), s));
  if ((e = bn254_launch_plonk_group_scatter(k.st, m, k.grp_st, k.d_fail, s)) != hipSuccess) return launch_err(e, "pairing RLC group scatter");
  HIPCK(hipMemcpyAsync(k.h_fail, k.d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  const uint32_t failed = *(const uint32_t*)k.h_fail;
  g_pbr_state[0].fetch_add(1, std::memory_order_relaxed); g_pbr_state[1].fetch_add(groups, std::memory_order_relaxed); g_pbr_state[2].fetch_add(failed, std::memory_order_relaxed);
  // the items of a failed group are still pending, on their weighted points: the exact check runs on exactly those wavefronts (every kernel of the pairing batch
  // leaves a wavefront without a pending item at once)
  if (failed && (rc = pbr_exact(d, nullptr, 0, n_pairs, sh, m, d.ws, k.st, true, force, nullptr, s))) return rc;
  HIPCK(hipMemcpyAsync(d_status, k.st, m, hipMemcpyDeviceToDevice, s));
  return BN254_OK;
}
int pbr_fresh_key(bn254::ChaChaKey& key) {
  uint32_t words[11];
  for (size_t got = 0; got < sizeof words;) {
    const ssize_t q = getrandom((uint8_t*)words + got, sizeof words - got, 0);
    if (q <= 0) return set_err(BN254_E_HIP, "getrandom failed: no weights for the pairing batch");
    got += (size_t)q;
  }
  for (int i = 0; i < 8; i++) key.k[i] = words[i];
  for (int i = 0; i < 3; i++) key.nonce[i] = words[8 + i];
  return BN254_OK;
}
// the launches of a call on device memory: caller holds d.mu and has run pbr_ensure(weighted: some launch may be).  A launch of rlc_min items or more of an honoured
// shape takes the weighted form (rlc_min SIZE_MAX: none); the weights of launch j come from the call's key with the launch number in a nonce word
int pbr_enqueue(PbDev& d, PbrDev& k, const uint8_t* d_items, size_t stride, size_t n_pairs, const PbShared& sh, size_t n, uint8_t* d_status, size_t rlc_min, int force, hipStream_t s,
                const uint32_t* d_weights = nullptr, const PbrProbeDev* pr = nullptr) {
  const size_t cap = d.ws_items();
  if (cap == 0) return set_err(BN254_E_BAD_ARG, "pairing workspace not allocated (internal sizing error)");
  if (d.busy_valid) HIPCK(hipStreamWaitEvent(s, d.busy_ev, 0));
  bn254::ChaChaKey wkey;
  memset(&wkey, 0, sizeof wkey);
  bool have_key = false;
  int rc = BN254_OK;
  uint32_t pass = 0;
  for (size_t off = 0; off < n && !rc; off += cap, pass++) {
    const size_t m = n - off < cap ? n - off : cap;
    const bool weighted = pr != nullptr || (rlc_min != SIZE_MAX && pbr_honoured(n_pairs, sh.mask, m, rlc_min));
    if (!weighted) {
      if (!(rc = pbr_exact(d, d_items + off * stride, stride, n_pairs, sh, m, d.ws, d_status + off, false, force, nullptr, s))) g_pbr_state[3].fetch_add(1, std::memory_order_relaxed);
      continue;
    }
    if (!d_weights && !have_key) { if ((rc = pbr_fresh_key(wkey))) break; have_key = true; }
    bn254::ChaChaKey pk = wkey;
    pk.nonce[2] ^= pass;
    rc = pbr_launch(d, k, d_items + off * stride, stride, n_pairs, sh, m, d_status + off, d_weights ? d_weights + 4 * off : nullptr, pk, force, s, pr);
  }
  // also after a failure: whatever was enqueued must be behind the event the next call waits for
  const hipError_t e = hipEventRecord(d.busy_ev, s);
  if (e == hipSuccess) d.busy_valid = true;
  if (!rc && e != hipSuccess) return set_err(BN254_E_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
  return rc;
}
// a probe's weight: 16 big-endian bytes -> four little-endian words, forced odd (bn254_capi_kzg.hip::kzg_weight_words)
void pbr_weight_words(uint32_t w[4], const uint8_t* be16) {
  for (int q = 0; q < 4; q++) { const uint8_t* b = be16 + 4 * (3 - q); w[q] = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | (uint32_t)b[3]; }
  w[0] |= 1u;
}
// what the launch leaves of an item's status: the groups' verdict for an item that reached them, the exact check of a failed group's item
uint8_t pbr_final_status(uint8_t st_mid, uint8_t grp_st, uint8_t st_item) {
  if (!(st_mid & BN254_ST_PENDING)) return st_mid;
  return grp_st == BN254_ST_ACCEPT ? (uint8_t)BN254_ST_ACCEPT : st_item;
}

// a host-buffer call: the pinned staging of the pairing entries, one pass at a time (the prepared records in front of every pass's items, packed; the probe's weights
// behind them).  ph: the probe (one pass)
struct PbrProbeHost { uint8_t *item_gt, *grp_gt, *grp_st; };
int pbr_host_call(const uint8_t* items, size_t item_stride, size_t n_pairs, const PbShared& sh, size_t n, uint8_t* status, int device, size_t rlc_min, int force, const uint8_t* weights,
                  const PbrProbeHost* ph) {
  PbDev* d = pb_dev(device);
  PbrDev* k = pbr_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  const size_t rec = bn254::pb_item_len((int)n_pairs, sh.mask), lead = sh.bytes(), wbytes = weights ? 16 : 0;
  const size_t pass = pb_host_pass_of(rec + wbytes, lead, n);
  static_assert(PB_PREP_LEN % 16 == 0 && PB_G1_LEN % 4 == 0 && PB_PAIR_LEN % 4 == 0, "the items behind the records and the weights behind the items stay dword-aligned");
  if (ph && n > pass) return set_err(BN254_E_BAD_ARG, "bad argument: the probe takes one pass");
  const bool weighted = ph != nullptr || (rlc_min != SIZE_MAX && pbr_honoured(n_pairs, sh.mask, pass, rlc_min));
  int rc;
  if ((rc = pbr_ensure(*d, *k, device, pass, weighted)) || (rc = d->stream.ensure())) return rc;
  if ((rc = d->h_in.ensure(lead + pass * (rec + wbytes))) || (rc = d->d_in.ensure(lead + pass * (rec + wbytes))) || (rc = k->h_out.ensure(pass)) || (rc = k->d_out.ensure(pass))) return rc;
  hipStream_t s = d->stream;
  const size_t groups = (n + 63) / 64;
  DevBuf<uint8_t> probe_buf;
  PbrProbeDev pr{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (ph) {
    if ((rc = probe_buf.ensure(385 * groups + 386 * n))) return rc;
    uint8_t* b = probe_buf;
    pr.grp_gt = b; pr.item_gt = b + 384 * groups; pr.grp_st = b + 384 * (groups + n); pr.st_mid = pr.grp_st + groups; pr.st_item = pr.st_mid + n;
    HIPCK(hipMemsetAsync(b, 0, 385 * groups + 386 * n, s));
  }
  auto one_pass = [&](size_t off, size_t m) -> int {
    if (lead) memcpy(d->h_in, sh.prepared, lead);
    uint8_t* o = d->h_in + lead;
    if (item_stride == rec) parallel_copy(o, items + off * rec, m * rec);
    else for (size_t i = 0; i < m; i++) memcpy(o + i * rec, items + (off + i) * item_stride, rec);
    if (weights)
      for (size_t i = 0; i < m; i++) { uint32_t w4[4]; pbr_weight_words(w4, weights + 16 * (off + i)); memcpy(o + m * rec + 16 * i, w4, 16); }
    HIPCK(hipMemcpyAsync(d->d_in, d->h_in, lead + m * (rec + wbytes), hipMemcpyHostToDevice, s));
    const uint8_t* d_items = d->d_in + lead;
    int r = pbr_enqueue(*d, *k, d_items, rec, n_pairs, PbShared{sh.mask, sh.mask ? (const uint8_t*)d->d_in : nullptr}, m, k->d_out, rlc_min, force, s,
                        weights ? (const uint32_t*)(d_items + m * rec) : nullptr, ph ? &pr : nullptr);
    if (r) return r;
    if (ph) {
      std::vector<uint8_t> hb(385 * groups + 386 * n);
      HIPCK(hipMemcpy(hb.data(), probe_buf, hb.size(), hipMemcpyDeviceToHost));
      const uint8_t *g_st = hb.data() + 384 * (groups + n), *mid = g_st + groups, *item = mid + n;
      for (size_t g = 0; g < groups; g++) {      // a group without a pending item: the empty product (no kernel wrote it)
        bool any = false;
        for (size_t i = 64 * g; i < 64 * g + 64 && i < n; i++) any |= (mid[i] & BN254_ST_PENDING) != 0;
        if (!any) hb[384 * g + 31] = 1;
      }
      if (ph->grp_gt) memcpy(ph->grp_gt, hb.data(), 384 * groups);
      if (ph->item_gt) memcpy(ph->item_gt, hb.data() + 384 * groups, 384 * n);
      if (ph->grp_st) memcpy(ph->grp_st, g_st, groups);
      for (size_t i = 0; i < n; i++) status[i] = pbr_final_status(mid[i], g_st[i / 64], item[i]);
      return BN254_OK;
    }
    HIPCK(hipMemcpyAsync(k->h_out, k->d_out, m, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    memcpy(status + off, k->h_out, m);
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

// ---- the host compile: the loader, the weights, the Miller subset, the group sums and products and the checks on plain arrays (the probe with device -1) ----------
void pbr_host_gt(const bn254::PbHostLane& w, uint8_t* out) {
  using namespace bn254;
  const int korder[6] = {0, 2, 4, 1, 3, 5};
  for (int t = 0; t < 6; t++)
    for (int h = 0; h < 2; h++) { uint32_t v[8]; fp_to_words(v, w.ld(VE_S0 + 2 * korder[t] + h)); words_to_be(out + 64 * t + 32 * h, v); }
}
int pbr_on_host(const uint8_t* items, size_t stride, int np, uint32_t mask, const uint8_t* prepared, size_t n, const uint8_t* weights, const PbrProbeHost& ph, uint8_t* status) {
  using namespace bn254;
  static const PbHostKinds kinds;
  const uint32_t all = (1u << np) - 1u, sh = mask & all, var = all & ~sh;
  const int n_sh = __builtin_popcount(sh);
  std::vector<int32_t> recs((size_t)n_sh * PB_PREP_DWORDS + 1);      // the caller's bytes need not be aligned
  if (n_sh) memcpy(recs.data(), prepared, (size_t)n_sh * PB_PREP_LEN);
  const size_t groups = (n + 63) / 64;
  int run_steps = knob_run_steps_pairing_batch();
  if (run_steps < 1) run_steps = 1;
  const PbRecLines lines{recs.data()};
  std::vector<PbHostLane> ws(n), gws(groups);
  std::vector<uint8_t> st(n), gst(groups, BN254_ST_ACCEPT);
  const bool recs_ok = pb_records_ok(recs.data(), sh);
  for (size_t i = 0; i < n; i++) {
    PbHostLane& w = ws[i];
    for (auto& x : w.e) x = fp_zero();
    if (!recs_ok) { st[i] = BN254_ST_MALFORMED; continue; }
    st[i] = (uint8_t)(sh ? pb_load_item_shared(w, items + i * stride, np, sh, recs.data(), false) : pb_load_item(w, items + i * stride, np, false));
    if (!(st[i] & BN254_ST_PENDING)) continue;
    uint32_t wgt[4] = {1, 0, 0, 0};
    if (weights) pbr_weight_words(wgt, weights + 16 * i);
    pb_rlc_weigh_item(w, np, wgt, true);
    if (!var) continue;
    const uint32_t ident = pb_ident(w);
    int failed = -1;
    for (int s = 0; s < BN_ATE_STEPS; s += run_steps) {
      const int r = vm_miller_run_sub(w, kinds, s, s + run_steps < BN_ATE_STEPS ? s + run_steps : BN_ATE_STEPS, np, var, ident, VE_F, MR_FOLD_INIT | MR_FOLD_ATE);
      if (failed < 0) failed = r;
    }
    if (failed >= 0) st[i] = BN254_ST_NOT_IN_SUBGROUP;
  }
  int32_t one[12 * BN_NL] = {0};
  for (int l = 0; l < BN_NL; l++) one[l] = BN_ONE[l];
  for (size_t g = 0; g < groups; g++) {
    PbHostLane& gw = gws[g];
    for (auto& x : gw.e) x = fp_zero();
    if (ph.grp_gt) memset(ph.grp_gt + 384 * g, 0, 384);
    bool any = false;
    for (size_t i = 64 * g; i < 64 * g + 64 && i < n; i++) any |= (st[i] & BN254_ST_PENDING) != 0;
    if (!any) { if (ph.grp_gt) ph.grp_gt[384 * g + 31] = 1; continue; }      // the empty product
    uint32_t p_inf = 0;
    int t = 0;
    for (uint32_t m = sh; m; m &= m - 1, t++) {      // k_pairing_rlc_group_sums
      const int j = vp_first(m);
      G1Proj L = g1_identity();
      for (size_t i = 64 * g; i < 64 * g + 64 && i < n; i++) {
        if (!(st[i] & BN254_ST_PENDING) || ((pb_ident(ws[i]) >> (2 * j)) & 1u)) continue;
        G1Aff p; p.x = ws[i].ld(vp_p(j)); p.y = ws[i].ld(vp_p(j) + 1);
        L = g1_add(L, g1_from_affine(p));
      }
      const bool inf = g1_is_identity(L);
      G1Aff a = g1_to_affine(L);
      a.y = fp_select(inf, fp_one(), a.y);
      gw.st(vp_p(t), a.x); gw.st(vp_p(t) + 1, a.y);
      if (inf) p_inf |= 1u << t;
    }
    pb_rlc_group_finish(gw, sh, recs.data(), p_inf);
    if (var) {      // k_pairing_rlc_group_prod
      Fp12 f = fp12_one();
      for (size_t i = 64 * g; i < 64 * g + 64 && i < n; i++)
        if (st[i] & BN254_ST_PENDING) f = pb_rlc_mul12(f, pb_rlc_ld12(ws[i], VE_F));
      pb_rlc_st12(gw, sh ? (int)PB_RLC_FG_ELEM : (int)VE_F, f);
    }
    if (sh) {
      const uint32_t gident = pb_ident(gw);
      for (int s = 0; s < BN_ATE_STEPS; s += run_steps)
        vm_miller_run_mix<false>(gw, lines, kinds, s, s + run_steps < BN_ATE_STEPS ? s + run_steps : BN_ATE_STEPS, 0u, (1u << n_sh) - 1u, gident, VE_F, MR_FOLD_INIT | MR_FOLD_ATE);
      if (var) vm_f12_mul(gw, VE_F, VE_F, PB_RLC_FG_ELEM);
    }
    PbHostOps ops{gw};
    vm_final_exp_program(ops);
    if (ph.grp_gt) pbr_host_gt(gw, ph.grp_gt + 384 * g);
    gst[g] = vm_f12_eq_const(gw, VE_S0, one) ? BN254_ST_ACCEPT : BN254_ST_REJECT;
  }
  if (ph.grp_st) memcpy(ph.grp_st, gst.data(), groups);
  for (size_t i = 0; i < n; i++) {
    if (ph.item_gt) memset(ph.item_gt + 384 * i, 0, 384);
    uint8_t item = st[i];
    if (st[i] & BN254_ST_PENDING) item = pb_lane_shared_on_host(ws[i], np, sh, recs.data(), ph.item_gt ? ph.item_gt + 384 * i : nullptr, run_steps);
    status[i] = pbr_final_status(st[i], gst[i / 64], item);
  }
  return BN254_OK;
}

int pbr_check_flags(unsigned flags) {
  if (flags & ~(unsigned)BN254_FLAG_RLC) return set_err(BN254_E_BAD_ARG, "bad argument: flags other than BN254_FLAG_RLC");
  return BN254_OK;
}

}  // namespace

extern "C" {

int bn254_pairing_check_batch_flags(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared, size_t n, uint8_t* status, int device,
                                    unsigned flags) {
  int rc = pbr_check_flags(flags);
  if (rc) return rc;
  if (!flags) return bn254_pairing_check_batch_shared(items, item_stride, n_pairs, shared_mask, prepared, n, status, device);
  const PbShared sh{shared_mask, shared_mask ? prepared : nullptr};
  bool done;
  rc = pb_check_args(items, item_stride, n_pairs, n, status, nullptr, false, &done, PbShared{shared_mask, prepared}, true);
  if (rc || done) return rc;
  // ONE reading of the knob per call (bn254_set_pairing_rlc_params may run beside it)
  return pbr_host_call(items, item_stride, n_pairs, sh, n, status, device, (size_t)g_pbr_rlc_min.load(std::memory_order_relaxed), bn254::PAIRING_FORM_PLAN, nullptr, nullptr);
}

int bn254_pairing_check_batch_flags_device(const void* d_items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const void* d_prepared, size_t n, void* d_status, int device,
                                           void* hip_stream, unsigned flags) {
  int rc = pbr_check_flags(flags);
  if (rc) return rc;
  if (!flags) return bn254_pairing_check_batch_shared_device(d_items, item_stride, n_pairs, shared_mask, d_prepared, n, d_status, device, hip_stream);
  const PbShared sh{shared_mask, shared_mask ? (const uint8_t*)d_prepared : nullptr};
  bool done;
  rc = pb_check_args(d_items, item_stride, n_pairs, n, d_status, nullptr, false, &done, PbShared{shared_mask, (const uint8_t*)d_prepared}, false);
  if (rc || done) return rc;
  PbDev* d = pb_dev(device);
  PbrDev* k = pbr_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  // below the knob (or for a shape the flag is not honoured for) nothing is allocated when a reservation of min(n, 2^18) items stands and the call only enqueues; the
  // weighted form grows its own buffers, and synchronises anyway
  const size_t rlc_min = (size_t)g_pbr_rlc_min.load(std::memory_order_relaxed);
  const bool weighted = pbr_honoured(n_pairs, sh.mask, n, rlc_min);
  if ((rc = pbr_ensure(*d, *k, device, n, weighted))) return rc;
  return pbr_enqueue(*d, *k, (const uint8_t*)d_items, item_stride, n_pairs, sh, n, (uint8_t*)d_status, weighted ? rlc_min : SIZE_MAX, bn254::PAIRING_FORM_PLAN, (hipStream_t)hip_stream);
}

void bn254_set_pairing_rlc_params(long rlc_min) {
  if (rlc_min >= 0) g_pbr_rlc_min.store(pbr_rlc_clamp(rlc_min));
}
int bn254_pairing_rlc_params(long out[1]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  out[0] = g_pbr_rlc_min.load();
  return BN254_OK;
}
int bn254_pairing_rlc_state(uint64_t out[4]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  for (int i = 0; i < 4; i++) out[i] = g_pbr_state[i].load(std::memory_order_relaxed);
  return BN254_OK;
}

// test-only: the bound on the variable positions of a shape the flag is honoured for (0 .. 8; negative: the default); returns the value it replaces
int bn254_dbg_set_pairing_rlc_max_var(int max_var) {
  return g_pbr_max_var.exchange(max_var < 0 ? PBR_MAX_VAR_HONOURED : max_var > 8 ? 8 : max_var);
}

// The probe: ONE weighted launch whatever the knob and the shape, with the caller's weights (n x 16 bytes big-endian, forced odd; null: the real draw on a device, all 1
// in the host compile).  out_item_gt (n x 384, may be null): the final-exponentiated value of every item that reached the groups, on its weighted points (zero
// otherwise); out_group_gt (ceil(n / 64) x 384) and out_group_status: the value and the verdict of every group (1 and ACCEPT for a group without a pending item);
// status: what the entry answers.  device -1 (form 0): the host compile of the same bodies; a device ordinal: the kernels, form 0 as the plan says, 1 the lane kernels,
// 2 the cooperative kernel for the group check and the exact check (the Miller runs of the items take the lane form at every size)
int bn254_dbg_pairing_batch_rlc(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared, size_t n, const uint8_t* weights,
                                uint8_t* out_item_gt, uint8_t* out_group_gt, uint8_t* out_group_status, uint8_t* status, int device, int form) {
  const PbShared sh{shared_mask, shared_mask ? prepared : nullptr};
  bool done;
  int rc = pb_check_args(items, item_stride, n_pairs, n, status, nullptr, false, &done, PbShared{shared_mask, prepared}, true);
  if (rc) return rc;
  if (device < -1 || form < 0 || form > bn254::PAIRING_FORM_COOP || (form != bn254::PAIRING_FORM_PLAN && device < 0))
    return set_err(BN254_E_BAD_ARG, "bad argument: form 0 runs anywhere, form 1 (lane) and 2 (cooperative) run on a device");
  if (form == bn254::PAIRING_FORM_COOP && n > (size_t)COOP12_MAX_PROOFS) return set_err(BN254_E_BAD_ARG, "bad argument: the cooperative form takes at most 30 720 items");
  if (done) return BN254_OK;
  const PbrProbeHost ph{out_item_gt, out_group_gt, out_group_status};
  if (device >= 0) return pbr_host_call(items, item_stride, n_pairs, sh, n, status, device, SIZE_MAX, form, weights, &ph);
  return pbr_on_host(items, item_stride, (int)n_pairs, sh.mask, sh.prepared, n, weights, ph, status);
}

}  // extern "C"
