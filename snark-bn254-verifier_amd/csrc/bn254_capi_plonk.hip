// bn254_capi_plonk.hip -- the PlonK half of the C ABI (include/bn254_verify.h): the key's device tables and context pool, the batch plan, the pass
// (plonk_pass: every stage on the device, bn254_k_plonk.hip and bn254_k_msm.hip; the one pass of single keys and of key lists, bn254_capi_plonk_keys.hip) with the
// worker loop that runs the passes of a plan, and every bn254_plonk_* entry on one key.
#include "bn254_capi_internal.h"

#define PLONK_BIG_PIECE_DEFAULT 131072   // proofs per pass of a batch above 65 536 proofs (profiles/r05_plonk_piece_sweep.txt)

int plonk_ensure_dev(const bn254_plonk_pvk* pvk, int device, PlonkDev** out) {
  int rc = check_device(device);
  if (rc || (rc = selftest_gate(device))) return rc;
  PlonkDev& d = pvk->dev[device];
  if (!d.ready) {
    if ((rc = upload(d.tab0, pvk->tab0)) || (rc = upload(d.tab1, pvk->tab1)) || (rc = upload(d.one, pvk->one))) return rc;
    if ((rc = build_tables_on_device(2, pvk->fixed_pts, d.fixed_tabs))) return rc;
    // the key and the field constants for the device-side stages
    if (sizeof(PlonkKey) != bn254_plonk_key_bytes()) return set_err(BN254_E_HIP, "PlonK key layout differs between the translation units");
    HIPCK(bn254_plonk_dev_init(device));
    if ((rc = d.d_key.ensure(sizeof(PlonkKey)))) return rc;
    HIPCK(hipMemcpy(d.d_key, &pvk->key, sizeof(PlonkKey), hipMemcpyHostToDevice));
    // known-answer check of the device stages on this GPU before the key is used there (bn254_k_plonk.hip::bn254_plonk_self_test); BN254_PLONK_SELFTEST=0 skips it
    static const bool selftest = [] { const char* e = getenv("BN254_PLONK_SELFTEST"); return !e || atoi(e) != 0; }();
    if (selftest) {
      std::string why;
      HIPCK(bn254_plonk_self_test(&pvk->key, d.d_key, &why));
      if (!why.empty()) return set_err(BN254_E_HIP, why);
    }
    d.ready = true;
  }
  *out = &d;
  return BN254_OK;
}
// Variable terms per JOINT row of an MSM launch over m_pad lanes per row (bn254_msm.h: Straus rows share the doublings of a step between their terms; 0 = one row per
// term).  A launch must still fill the GPU: two wavefronts per SIMD are 131 072 lanes, so joint rows pay from passes of tens of thousands of proofs on.
// BN254_MSM_JOINT=g forces a group size (0: never).
int plonk_joint_g(size_t m_pad) {
  static const int env = [] { const char* e = getenv("BN254_MSM_JOINT"); return e ? atoi(e) : -1; }();
  if (env >= 0) return env > MSM_MAX_JOINT ? MSM_MAX_JOINT : env;
  return m_pad >= 49152 ? MSM_MAX_JOINT : 0;      // measured (profiles/r04_msm_joint_rows_sweep.txt): all the terms of a sum in one row, from 49 152 proofs per pass
}
// lanes an MSM launch may use at one wavefront per SIMD: the planner splits variable terms over two rows while the launch stays within it (bn254_msm.h)
size_t msm_lane_budget() { static const size_t v = [] { const char* e = getenv("BN254_MSM_LANE_BUDGET"); long x = e ? atol(e) : 65536; return (size_t)(x < 64 ? 64 : x); }(); return v; }
// Lanes of window-table scratch a context of capacity `need` proofs must hold: the largest launch ANY batch of up to `need` proofs can make with a launch of
// `n_var` variable terms -- split (2 n_var rows) while that stays within the budget, one row per term above.  (Rounds 2-3 sized the scratch from `need`
// itself while the launch form follows the batch's own size, and a 5000-proof batch on a 5120-proof context wrote 15 MB past the end.)
size_t plonk_scratch_lanes(size_t need, int n_var) {
  const size_t need_pad = (need + 63) & ~(size_t)63, b = msm_lane_budget() / 64 * 64;
  size_t split = 2 * (size_t)n_var * need_pad; if (split > b) split = b;
  const size_t full = (size_t)n_var * need_pad;
  return split > full ? split : full;
}
// Points (rows x items) the row buffer of a context of capacity `need` must hold for launches of `shape`: a split launch (latency form) has at most lane_budget / n_pad rows,
// so rows x items stays within the lane budget; an unsplit one has the rows of its shape's plan without joint rows (joint rows only merge rows), whatever the item count.
size_t plonk_part_points(size_t need, const MsmShape& shape) {
  MsmPlan big;
  if (!msm_plan_build(big, shape, 64, 0, 0, 0)) return need * (size_t)MSM_MAX_ROWS;
  const size_t need_pad = (need + 63) & ~(size_t)63;
  // (a sum without variable terms, or an empty one, takes one row even when the budget has none left: two sums, two rows beyond the budget at most)
  size_t split = msm_lane_budget() + 2 * need_pad; if (split > need_pad * (size_t)MSM_MAX_ROWS) split = need_pad * (size_t)MSM_MAX_ROWS;
  const size_t full = (size_t)big.n_rows * need_pad;
  return split > full ? split : full;
}
static int shape_var(const MsmShape& sh) { int v = 0; for (int s = 0; s < sh.n_sums; s++) v += sh.n_var[s]; return v; }
// Knobs of the PlonK batch plan (bn254_set_plonk_params; the environment gives their initial values once, at load time):
//   piece      proofs per pass while a batch is a set of latency-bound chains side by side (5040: every launch of a pass is one wavefront generation and the
//              MSM launches keep their split form)
//   workers    sub-batches in flight (contexts), at most PLONK_WORKERS
//   big_from   from this many proofs a batch runs as FEW LARGE passes instead (throughput: one row per variable term, fixed windows packed, the pairing check on
//              the lane kernels with the whole Miller loop in one launch): 65 536 proofs in one pass 2.28 M proofs/s against 1.48 M as eight chains of 5040-proof passes.
//              0 (default): the plan measured on the MI355X (plonk_auto_plan, profiles/r04_plonk_plan_sweep.txt)
//   big_piece  proofs per pass of that form (at most PLONK_MAX_LAUNCH)
static std::atomic<long> g_plonk_piece{[] { long v = env_long("BN254_PLONK_PIECE", 5040); return v < 256 ? 256 : (v > PLONK_MAX_LAUNCH ? (long)PLONK_MAX_LAUNCH : v); }()};
static std::atomic<int> g_plonk_workers{[] { long v = env_long("BN254_PLONK_WORKERS", PLONK_WORKERS); return (int)(v < 1 ? 1 : (v > PLONK_WORKERS ? PLONK_WORKERS : v)); }()};
static std::atomic<long> g_plonk_big_from{[] { long v = env_long("BN254_PLONK_BIG_FROM", 0); return v < 0 ? 0 : v; }()};      // 0: the measured plan of plonk_auto_plan
// BN254_FLAG_RLC on the PlonK entry: honoured from this many proofs per pass (BN254_PLONK_RLC_MIN gives the initial value)
static std::atomic<long> g_plonk_rlc_min{[] { long v = env_long("BN254_PLONK_RLC_MIN", 8192); return v < 64 ? 64 : v; }()};
size_t plonk_rlc_min() { return (size_t)g_plonk_rlc_min.load(); }
static std::atomic<long> g_plonk_big_piece{[] { long v = env_long("BN254_PLONK_BIG_PIECE", PLONK_BIG_PIECE_DEFAULT); return v < 256 ? 256 : (v > PLONK_MAX_LAUNCH ? (long)PLONK_MAX_LAUNCH : v); }()};
// the plan of a batch (bn254_plonk_verify_batch): sub-batches side by side, proofs per sub-batch, proofs per pass of a sub-batch
// The default plan by batch size (profiles/r04_plonk_plan_sweep.txt, one MI355X): chains of 5040-proof passes side by side up to ~9000 proofs (8192: 7.06 ms against
// 7.27 ms as one pass); ONE pass of the whole batch up to ~20 000 (16 384: 12.2 against 12.7 ms); TWO passes side by side up to ~40 000 (32 768: 18.3 ms against 20.2 ms
// as one pass and 22.3 ms as chains); one pass again up to 65 536 (49 152: 25.1 ms = 1.96 M proofs/s, 65 536: 28.8 ms = 2.28 M, chains 1.48 M); beyond, passes of up to
// big_piece proofs (bn254_set_plonk_params; default PLONK_BIG_PIECE_DEFAULT) on up to eight contexts (round 4, passes of 65 536: 262 144 proofs at 2.62 M proofs/s).
static void plonk_auto_plan(size_t n, size_t chain_piece, size_t big_piece, int max_workers, size_t* piece, int* workers_cap) {
  if (n <= 9000) { *piece = chain_piece; *workers_cap = max_workers; }
  else if (n <= 20000) { *piece = n; *workers_cap = 1; }
  else if (n <= 40000) { *piece = (n + 1) / 2; *workers_cap = max_workers < 2 ? max_workers : 2; }
  else if (n <= 65536) { *piece = n; *workers_cap = max_workers; }
  else { *piece = n < big_piece ? n : big_piece; *workers_cap = max_workers; }
}
void plonk_plan(size_t n, size_t piece, int max_workers, int* workers, size_t* per, size_t* pass) {
  int w = (int)((n + piece - 1) / piece); if (w > max_workers) w = max_workers; if (w < 1) w = 1;
  const size_t p = (n + (size_t)w - 1) / (size_t)w;
  const size_t npass = (p + piece - 1) / piece;
  *workers = w; *per = p; *pass = npass ? (p + npass - 1) / npass : p;
}
// n: proofs of the largest pass the context will run; in_bytes: the proof + input bytes of such a pass (device-side stages: staged through pinned memory).  Everything a pass
// needs is sized HERE, before anything is enqueued: the run path itself neither allocates nor frees (a hipFree is a device-wide synchronisation while other contexts are in flight).
int plonk_ensure_ctx(const bn254_plonk_pvk* pvk, PlonkCtx& c, size_t n, size_t in_bytes) {
  int rc;
  if ((rc = c.stream.ensure()) || (rc = c.aux.ensure()) || (rc = c.ev_fork.ensure()) || (rc = c.ev_join.ensure())) return rc;
  for (auto& e : c.tk) if ((rc = e.ensure_timed())) return rc;
  if (in_bytes > c.in_cap()) {   // the staging pair: both, or neither
    const size_t cap = (in_bytes + 65535) / 65536 * 65536;
    c.h_in.release();
    if ((rc = c.d_in.ensure(cap)) || (rc = c.h_in.ensure(cap))) { c.d_in.release(); return rc; }
  }
  size_t need = n < PLONK_MAX_LAUNCH ? (n + 255) / 256 * 256 : (size_t)PLONK_MAX_LAUNCH;
  if (need <= c.cap) return BN254_OK;
  // The buffers of a pass are sized together for c.cap proofs, or not at all: the old ones go BEFORE anything is allocated, and if an allocation below fails the
  // context is left empty (cap = 0, every buffer empty)
  auto drop = [&c] {
    c.ws.release(); c.part.release(); c.glv_tab.release(); c.terms.release(); c.flags.release(); c.words.release(); c.inf.release(); c.status.release(); c.d_work.release();
    c.grp_ws.release(); c.grp_status.release(); c.d_fail.release(); c.h_status.release(); c.h_fail.release();
    c.cap = 0; c.glv_lanes = 0; c.part_points = 0;
  };
  drop();
  const int T1 = plonk_stage1_terms(pvk->key), TT = plonk_stage2_terms(pvk->key) + 2;
  const size_t tmax = (size_t)(TT > T1 ? TT : T1);
  // window-table scratch of the variable rows: the bound over every batch size up to `need` and both launches (plonk_scratch_lanes)
  const int v1 = shape_var(pvk->shape1), v2 = shape_var(pvk->shape2_rlc);        // (the weighted form of the second launch has one variable term more)
  const size_t tab_lanes = plonk_scratch_lanes(need, v1 > v2 ? v1 : v2);
  size_t pp = plonk_part_points(need, pvk->shape1);                              // one projective point per row and item of a launch's plan
  { const size_t b = plonk_part_points(need, pvk->shape2), c2 = plonk_part_points(need, pvk->shape2_rlc); if (b > pp) pp = b; if (c2 > pp) pp = c2; }
  const size_t groups = (need / 64 + 255) / 256 * 256;                             // need is a multiple of 256: need / 64 groups, rounded to whole workgroups
  if ((rc = c.ws.ensure(need * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = c.part.ensure(pp * 27)) ||
      (rc = c.glv_tab.ensure(tab_lanes * (size_t)(G1_GLV_TAB_BYTES_PER_LANE / 4))) ||       // 65536 lanes = 117 MB for capacities up to 8192 proofs
      (rc = c.terms.ensure(need * tmax)) || (rc = c.flags.ensure(need * tmax)) || (rc = c.words.ensure(need * 16)) || (rc = c.inf.ensure(need)) || (rc = c.status.ensure(need)) ||
      (rc = c.d_work.ensure(need * bn254_plonk_work_bytes())) || (rc = c.grp_ws.ensure(groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = c.grp_status.ensure(groups)) ||
      (rc = c.d_fail.ensure(1)) || (rc = c.h_status.ensure(need)) || (rc = c.h_fail.ensure(1))) {
    drop();
    return rc;
  }
  c.part_points = pp; c.glv_lanes = tab_lanes; c.cap = need;
  return BN254_OK;
}

static KeyCache<bn254_plonk_pvk, bn254_plonk_vk_free>& plonk_key_cache() { static auto* c = new KeyCache<bn254_plonk_pvk, bn254_plonk_vk_free>(); return *c; }

extern "C" {

// ---------------------------------------------------------------- PlonK (BASELINE configs[3]): entry points
int bn254_plonk_vk_prepare(const uint8_t* vk, size_t vk_len, bn254_plonk_pvk** out) {
  if (!vk || !out) return set_err(BN254_E_BAD_ARG, "bad argument");
  *out = nullptr;
  auto* p = new bn254_plonk_pvk();
  if (parse_plonk_vk(p->key, vk, vk_len) != DEC_OK) { delete p; return set_err(BN254_E_VK, "PlonK verifying key does not parse"); }
  // line tables of the two KZG G2 points (kzg.rs:175-187: e(P0, g2[0]) e(P1, g2[1]) == 1); target = 1 in GT
  std::vector<FixedLine> t0(BN_ATE_STEPS), t1(BN_ATE_STEPS);
  if (!fixed_line_table(t0.data(), p->key.kzg_g2[0]) || !fixed_line_table(t1.data(), p->key.kzg_g2[1])) { delete p; return set_err(BN254_E_VK, "no line table for a KZG G2 point (unreachable for a point on the twist: bn254_host.hpp::prepare_g16)"); }
  p->tab0.resize((size_t)BN_ATE_STEPS * FIXED_LINE_DWORDS); p->tab1.resize((size_t)BN_ATE_STEPS * FIXED_LINE_DWORDS);
  for (int s = 0; s < BN_ATE_STEPS; s++) {
    int32_t* a = p->tab0.data() + (size_t)s * FIXED_LINE_DWORDS; int32_t* b = p->tab1.data() + (size_t)s * FIXED_LINE_DWORDS;
    put_fp2(a, t0[s].m); put_fp2(a + 2 * BN_NL, t0[s].c); put_fp2(a + 4 * BN_NL, t0[s].xc);
    put_fp2(b, t1[s].m); put_fp2(b + 2 * BN_NL, t1[s].c); put_fp2(b + 4 * BN_NL, t1[s].xc);
  }
  p->one.resize(12 * BN_NL);
  put_fp12(p->one.data(), fp12_one());
  // byte-window tables of the key's G1 points that enter the MSMs with per-proof scalars (plonk/verify.rs:253-284: ql, qr, qm, qo, qk, s3; plonk/kzg.rs:74-85:
  // s1, s2, qcp[]; kzg.rs:169: the KZG generator): 32 mixed additions per term instead of a 128-step double-and-add chain
  {
    // built on the device that uses them (bn254_k_comb.hip form 2: MSM_FW_WINDOWS windows of MSM_FW_BITS bits, bn254_fw.h): the host keeps the points
    const int nt = plonk_num_tables(p->key);
    p->fixed_pts.resize((size_t)nt * 2 * BN_NL);
    for (int i = 0; i < nt; i++) { const G1Aff& q = plonk_table_point(p->key, i); fp_to_limbs(p->fixed_pts.data() + (size_t)i * 2 * BN_NL, q.x); fp_to_limbs(p->fixed_pts.data() + (size_t)i * 2 * BN_NL + BN_NL, q.y); }
  }
  plonk_msm1_shape(p->key, p->shape1); plonk_msm2_shape(p->key, p->shape2); plonk_msm2_shape(p->key, p->shape2_rlc, true);
  *out = p;
  return BN254_OK;
}
void bn254_plonk_vk_free(bn254_plonk_pvk* pvk) {
  if (!pvk) return;
  plonk_keys_sets_drop(pvk);      // every cached key set that contains it (their descriptors point into the device state released below)
  for (auto it = pvk->dev.begin(); it != pvk->dev.end();) {
    if (hipSetDevice(it->first) != hipSuccess) { ++it; continue; }   // (its state goes with the key below, without the wait)
    (void)hipDeviceSynchronize();
    it = pvk->dev.erase(it);      // the state's members release what they own on the device that is now current and idle
  }
  delete pvk;
}
size_t bn254_plonk_vk_num_public(const bn254_plonk_pvk* pvk) { return pvk ? (size_t)pvk->key.nb_public : 0; }

}  // extern "C"

// One MSM launch of a sub-batch: plan the rows for this batch size (bn254_msm.h: a pure function of the launch's term kinds, the item count and the lane
// budget), check the plan against what the context holds -- the launch form follows the BATCH, the buffers the context's CAPACITY -- and enqueue rows + sums.
// Over a key list (bn254_capi_plonk_keys.hip) the items are slots and the window tables are those of every granule's key
int plonk_msm(const PlonkTables& t, PlonkCtx& c, const MsmShape& shape, size_t m, int n_terms, bool to_words, size_t* lanes_out, hipEvent_t ev_rows) {
  MsmPlan plan;
  const size_t m_pad = (m + 63) & ~(size_t)63;
  // BN254_MSM_SPLIT_AT (experiments): the bit position at which the variable terms' low and high rows meet, instead of the planner's choice
  static const int force_a = [] { const char* e = getenv("BN254_MSM_SPLIT_AT"); int v = e ? atoi(e) : 0; return (v >= 2 && v <= 126 && !(v & 1)) ? v : 0; }();
  if (!msm_plan_build(plan, shape, m_pad, msm_lane_budget(), force_a, plonk_joint_g(m_pad))) return set_err(BN254_E_BAD_ARG, "PlonK key shape needs more MSM rows than the launch supports");
  if (m > c.cap || bn254_g1_msm_scratch_lanes(plan, m) > c.glv_lanes || (size_t)plan.n_rows * m > c.part_points || (size_t)plan.n_rows > (size_t)MSM_MAX_ROWS)
    return set_err(BN254_E_HIP, "PlonK context smaller than the launch (internal sizing error)");
  hipError_t e = t.desc ? bn254_launch_g1_msm_rows_keys(plan, (const int32_t*)(MsmTerm*)c.terms, c.flags, m, n_terms, c.part, c.glv_tab, t.desc, t.n_keys, t.granule_key, c.stream)
                        : bn254_launch_g1_msm_rows(plan, (const int32_t*)(MsmTerm*)c.terms, c.flags, m, n_terms, c.part, c.glv_tab, t.key->fixed_tabs, c.stream);
  if (ev_rows) HIPCK(hipEventRecord(ev_rows, c.stream));
  if (e == hipSuccess)
    e = to_words ? bn254_launch_g1_sum_rows(plan, c.part, m, c.words, c.inf, nullptr, nullptr, 0, 0, 0, 0, c.stream)
                 : bn254_launch_g1_sum_rows(plan, c.part, m, nullptr, nullptr, c.ws, c.status, VE_LX_ELEM, BN254_ST_LINF, VE_CX_ELEM, BN254_ST_LINF2, c.stream);
  if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("MSM launch: ") + hipGetErrorString(e));
  if (lanes_out) *lanes_out = (size_t)plan.n_rows * m_pad;
  return BN254_OK;
}
// The other launches of a pass that differ between one key and a list: each picks the launcher and hands it its arguments, nothing else.
int PlonkTables::launched(hipError_t e, const char* what) const {
  if (e == hipSuccess) return BN254_OK;
  return desc ? launch_err(e, what) : set_err(BN254_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
}
static int pass_stage1(const PlonkTables& t, const PlonkPassIn& in, PlonkCtx& c, size_t m, const uint32_t lam_key[11], int T1) {
  return t.launched(t.desc ? bn254_launch_plonk_stage1_keys(t.desc, t.n_keys, t.granule_key, in.recs, in.rec_stride, in.proof_len, in.inputs, in.in_stride, in.staged_public, m, lam_key,
                                                            c.d_work, c.terms, c.flags, T1, c.stream)
                           : bn254_launch_plonk_stage1(t.key->d_key, in.recs, in.rec_stride, in.inputs, in.n_public, m, lam_key, c.d_work, c.terms, c.flags, T1, c.stream),
                    "PlonK stage 1");
}
static int pass_stage2(const PlonkTables& t, const PlonkPassIn& in, PlonkCtx& c, size_t m, int TT, int T2, const uint32_t* weight_key) {
  return t.launched(t.desc ? bn254_launch_plonk_stage2_keys(t.desc, t.n_keys, t.granule_key, in.recs, in.rec_stride, m, c.d_work, c.words, c.inf, c.terms, c.flags, c.status, TT, T2,
                                                            weight_key, c.stream)
                           : bn254_launch_plonk_stage2(t.key->d_key, in.recs, in.rec_stride, m, c.d_work, c.words, c.inf, c.terms, c.flags, c.status, TT, T2, weight_key, c.stream),
                    "PlonK stage 2");
}
// the pairing check of every pending proof: over a list in the form that follows the pass's size (bn254_set_plonk_keys_params: cooperative with the key per item, or
// the lane form with the key per wavefront)
static hipError_t pass_check_items(const PlonkTables& t, PlonkCtx& c, size_t m) {
  return t.desc ? bn254_launch_pairing2_fixed_keys(c.ws, c.status, m, t.desc, t.n_keys, t.granule_key, t.one, BN254_ERR_PAIRING_FAILED, c.stream)
                : bn254_launch_pairing2_fixed(c.ws, c.status, m, t.key->tab0, t.key->tab1, t.one, BN254_ERR_PAIRING_FAILED, c.stream, c.aux, c.ev_fork, c.ev_join);
}
// the pairing check of every group of 64.  Over a list a group is a granule, so all its proofs have one key, and group g of the pass is checked against the tables of
// granule g
static hipError_t pass_check_groups(const PlonkTables& t, PlonkCtx& c, size_t groups) {
  return t.desc ? bn254_launch_pairing2_fixed_groups_keys(c.grp_ws, c.grp_status, groups, t.desc, t.n_keys, t.granule_key, t.one, BN254_ERR_PAIRING_FAILED, c.stream)
                : bn254_launch_pairing2_fixed(c.grp_ws, c.grp_status, groups, t.key->tab0, t.key->tab1, t.one, BN254_ERR_PAIRING_FAILED, c.stream, c.aux, c.ev_fork, c.ev_join);
}

// The KZG batching scalar of every proof: fresh, uniform and unpredictable to the prover, as the reference draws it
// (Fr::random(&mut OsRng), plonk/kzg.rs:149-154).  It MUST be secret until the proof is fixed: the two opening quotients are bound by
// no transcript, so a prover who knows lambda can shift them by (lambda D, -D) and cancel a wrong evaluation
// (tests/test_oracle_golden.py::test_kzg_batching_scalar_must_be_unpredictable).  A ChaCha20 key and nonce from getrandom(2) per pass;
// k_plonk_stage1 gives proof i the 384 bits of blocks 3i .. 3i+2 reduced mod r.
static int plonk_fresh_lam_key(uint32_t lam_key[11]) {
  for (size_t got = 0; got < 11 * sizeof(uint32_t);) {
    ssize_t k = getrandom((uint8_t*)lam_key + got, 11 * sizeof(uint32_t) - got, 0);
    if (k <= 0) return set_err(BN254_E_HIP, "getrandom failed: no KZG batching scalars");
    got += (size_t)k;
  }
  return BN254_OK;
}

// The first part of a pass, up to the row sums of the second MSM: stage 1 -> digest MSM -> stage 2 -> KZG MSM, all enqueued on c.stream.  It leaves the pairing
// operands of every pending proof at VE_LX / VE_CX of c.ws and the status bytes in c.status.  lam_key: the 11 words of the pass's ChaCha20 key and nonce; weighted: every
// scalar of both sums carries the proof's weight from the key's second stream (the form the joint check of BN254_FLAG_RLC needs).  The key is the CALLER's: plonk_pass
// below hands it a fresh one, and beside it only the value probes of bn254_capi_dbg.hip call this (tests/test_capi_cpu.py holds that).
int plonk_pass_points(const bn254_plonk_pvk* shapes, const PlonkTables& t, const PlonkPassIn& in, PlonkCtx& c, size_t m, const uint32_t lam_key[11], bool weighted, const Event* tk) {
  const int T1 = plonk_stage1_terms(shapes->key), T2 = plonk_stage2_terms(shapes->key), TT = T2 + 2;
  if (m > c.cap) return set_err(BN254_E_HIP, "PlonK context smaller than the pass (internal sizing error)");
  int rc;
  auto mark = [&](int k) { return tk ? hipEventRecord(tk[k], c.stream) : hipSuccess; };
  HIPCK(mark(0));
  if ((rc = pass_stage1(t, in, c, m, lam_key, T1))) return rc;
  HIPCK(mark(1));
  if ((rc = plonk_msm(t, c, shapes->shape1, m, T1, true, &c.last_lanes[0], tk ? (hipEvent_t)tk[2] : nullptr))) return rc;
  HIPCK(mark(3));
  if ((rc = pass_stage2(t, in, c, m, TT, T2, weighted ? lam_key : nullptr))) return rc;
  HIPCK(mark(4));
  if ((rc = plonk_msm(t, c, weighted ? shapes->shape2_rlc : shapes->shape2, m, TT, false, &c.last_lanes[1], tk ? (hipEvent_t)tk[5] : nullptr))) return rc;
  HIPCK(mark(6));
  return BN254_OK;
}

// One pass with BOTH host stages on the device (bn254_k_plonk.hip): the first part above under a fresh key, then the pairing check, on the context's stream, without
// a host wait in between unless BN254_FLAG_RLC is honoured.  Over a list a padding slot is decided by stage 1 and contributes the identity to everything after it.
int plonk_pass(const bn254_plonk_pvk* shapes, const PlonkTables& t, const PlonkPassIn& in, PlonkCtx& c, size_t m, unsigned flags, const Event* tk, PlonkPassReport* rep) {
  *rep = PlonkPassReport();
  if (m > c.cap) return set_err(BN254_E_HIP, "PlonK context smaller than the pass (internal sizing error)");
  uint32_t lam_key[11];
  int rc = plonk_fresh_lam_key(lam_key);
  if (rc) return rc;
  // BN254_FLAG_RLC: the pairing checks of the pass batched over groups of 64 proofs -- honoured from plonk_rlc_min proofs (slots) per pass (below, the one remaining
  // pairing is the same latency-bound launch as the per-proof checks and nothing is gained)
  const bool rlc = (flags & BN254_FLAG_RLC) != 0 && m >= plonk_rlc_min();
  const size_t groups = (m + 63) / 64;
  if (rlc && (groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4) > c.grp_ws.cap() || groups > c.grp_status.cap()))
    return set_err(BN254_E_HIP, "PlonK context smaller than the pass's groups (internal sizing error)");
  if ((rc = plonk_pass_points(shapes, t, in, c, m, lam_key, rlc, tk))) return rc;
  rep->exact = !rlc;
  if (rlc) {
    // group sums (weighted points of the 64 proofs of a wavefront) -> one pairing check per group -> pending proofs of passed groups accepted; the proofs of a
    // failed group stay pending and the exact check below runs on exactly their wavefronts (every other wavefront of its kernels exits at once)
    HIPCK(hipMemsetAsync(c.d_fail, 0, sizeof(uint32_t), c.stream));
    hipError_t e = bn254_launch_plonk_group_sums(c.ws, c.status, m, c.grp_ws, c.grp_status, VE_LX_ELEM, BN254_ST_LINF, VE_CX_ELEM, BN254_ST_LINF2, c.stream);
    if (e == hipSuccess) e = pass_check_groups(t, c, groups);
    if (e == hipSuccess) e = bn254_launch_plonk_group_scatter(c.status, m, c.grp_status, c.d_fail, c.stream);
    if ((rc = t.launched(e, "PlonK joint pairing check"))) return rc;
    HIPCK(hipMemcpyAsync(c.h_fail, c.d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    HIPCK(hipStreamSynchronize(c.stream));
    rep->joint = true; rep->groups = groups; rep->failed = *c.h_fail;
    rep->exact = rep->failed != 0;
  }
  if (rep->exact && (rc = t.launched(pass_check_items(t, c, m), "PlonK pairing check"))) return rc;
  if (tk) HIPCK(hipEventRecord(tk[7], c.stream));
  return BN254_OK;
}

extern "C" {

// One sub-batch of a batch on ONE key: one H2D copy of the proofs and inputs, the pass, one D2H copy of the status bytes.
// resident: proofs / public_inputs / status are DEVICE memory of `device` (bn254_plonk_verify_batch_device): no staging copy, the status bytes leave with a device-to-device copy.
// d_rows (SP1 public inputs): the pass's public inputs are already in device memory (n_public = 2), so with host buffers only the proofs are staged
static int plonk_run_device(const bn254_plonk_pvk* pvk, const PlonkDev* d, PlonkCtx& c, int device, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                            size_t n_public, size_t m, uint8_t* status, unsigned flags, bool resident, const uint8_t* d_rows = nullptr) {
  HIPCK(hipSetDevice(device));
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  auto t0 = now();
  const size_t pb = m * proof_stride, ib = d_rows ? 0 : m * n_public * 32, need = pb + ib;
  if (!resident && need > c.in_cap()) return set_err(BN254_E_HIP, "PlonK context staging smaller than the pass (internal sizing error)");   // sized by plonk_ensure_ctx
  if (!resident) {
    parallel_copy(c.h_in, proofs, pb);
    if (ib) parallel_copy(c.h_in + pb, public_inputs, ib);
  }
  auto t1_ = now();
  if (!resident) HIPCK(hipMemcpyAsync(c.d_in, c.h_in, need, hipMemcpyHostToDevice, c.stream));
  const uint8_t* d_proofs = resident ? proofs : c.d_in; const uint8_t* d_inputs = d_rows ? d_rows : resident ? public_inputs : c.d_in + pb;
  PlonkPassReport rep;
  int rc = plonk_pass(pvk, PlonkTables{d, nullptr, 0, nullptr, d->one}, PlonkPassIn{d_proofs, proof_stride, d_inputs, n_public, 0, 0, 0}, c, m, flags, c.tk, &rep);
  if (rc) return rc;
  if (resident) HIPCK(hipMemcpyAsync(status, c.status, m, hipMemcpyDeviceToDevice, c.stream));
  else HIPCK(hipMemcpyAsync(c.h_status, c.status, m, hipMemcpyDeviceToHost, c.stream));
  HIPCK(hipStreamSynchronize(c.stream));
  if (!resident) memcpy(status, c.h_status, m);
  {
    auto t4_ = now();
    // slots as bn254_plonk_last_timing names them; [0] is the host copy into pinned memory, everything else a kernel of the chain
    c.last_ms[0] = (float)ms(t0, t1_); c.last_ms[8] = (float)ms(t0, t4_);
    for (int k = 1; k <= 7; k++) HIPCK(hipEventElapsedTime(&c.last_ms[k], c.tk[k - 1], c.tk[k]));
    c.last_valid = true;
  }
  return BN254_OK;
}

int bn254_plonk_last_timing(const bn254_plonk_pvk* pvk, int device, float ms[BN254_PLONK_NUM_TIMINGS], size_t lanes[2]) {
  if (!pvk || !ms) return set_err(BN254_E_BAD_ARG, "bad argument");
  PlonkDev* d = nullptr;
  {
    std::lock_guard<std::mutex> lk(pvk->mu);
    auto it = pvk->dev.find(device);
    if (it != pvk->dev.end()) d = &it->second;
  }
  if (!d) return set_err(BN254_E_BAD_ARG, "no PlonK batch on this device yet");
  std::lock_guard<std::mutex> lk(d->pool_mu);
  if (!d->last_valid) return set_err(BN254_E_BAD_ARG, "no PlonK batch on this device yet");
  for (int i = 0; i < BN254_PLONK_NUM_TIMINGS; i++) ms[i] = d->last_ms[i];
  if (lanes) { lanes[0] = d->last_lanes[0]; lanes[1] = d->last_lanes[1]; }
  return BN254_OK;
}

}  // extern "C"

// the plan of a batch of n proofs under the current knobs: sub-batches side by side, proofs per sub-batch, proofs per pass
// piece: the most proofs a pass of a batch of n may hold; *max_workers: the most sub-batches side by side
size_t plonk_piece_for(size_t n, int* max_workers) {
  *max_workers = g_plonk_workers.load();
  size_t piece;
  const long big_from = g_plonk_big_from.load();
  if (big_from == 0) plonk_auto_plan(n, (size_t)g_plonk_piece.load(), (size_t)g_plonk_big_piece.load(), *max_workers, &piece, max_workers);
  else piece = n >= (size_t)big_from ? (size_t)g_plonk_big_piece.load() : (size_t)g_plonk_piece.load();
  return piece;
}
void plonk_plan_for(size_t n, int* workers, size_t* per, size_t* pass_cap) {
  int max_workers;
  const size_t piece = plonk_piece_for(n, &max_workers);
  plonk_plan(n, piece, max_workers, workers, per, pass_cap);
}
// the batch sizes that END a segment of the plan: within a segment the piece and the worker count do not fall as n grows (plonk_auto_plan, or big_from)
int plonk_plan_breaks(size_t out[4]) {
  const long big_from = g_plonk_big_from.load();
  if (big_from == 0) { out[0] = 9000; out[1] = 20000; out[2] = 40000; out[3] = 65536; return 4; }
  if (big_from > 1) { out[0] = (size_t)big_from - 1; return 1; }
  return 0;
}

int plonk_run_workers(const PlonkLease& lease, int workers, size_t per, size_t pass, size_t total, const std::function<int(int, size_t, size_t)>& run_pass) {
  std::vector<int> rcs(workers, BN254_OK); std::vector<std::string> errs(workers);
  auto body = [&](int w) {
    const size_t lo = (size_t)w * per, hi = lo + per < total ? lo + per : total;
    for (size_t off = lo; off < hi; off += pass) {
      int r = run_pass(w, off, hi - off < pass ? hi - off : pass);
      if (r) {
        // work of this pass may still be enqueued on the context's streams: drain them before the lease hands the context (its staging, its term and status
        // buffers) to the next call
        rcs[w] = r; errs[w] = g_err;
        (void)hipStreamSynchronize(lease.ctx(w).stream); (void)hipStreamSynchronize(lease.ctx(w).aux);
        return;
      }
    }
  };
  if (workers == 1) body(0);
  else {
    std::vector<std::thread> th;
    for (int w = 0; w < workers; w++) th.emplace_back(body, w);
    for (auto& t : th) t.join();
  }
  for (int w = 0; w < workers; w++) if (rcs[w]) return set_err(rcs[w], errs[w]);
  return BN254_OK;
}

// One batch.  resident = false: proofs / public_inputs / status are the caller's host buffers (each pass stages its share through the context's pinned memory);
// resident = true: they are device memory of `device` and nothing is staged.  Either way the call returns when every status byte is where the caller asked for it.
// d_rows: see plonk_run_device (public_inputs is then ignored and n_public must be 2)
static int plonk_batch(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n, uint8_t* status,
                       int device, unsigned flags, bool resident, const uint8_t* d_rows = nullptr) {
  PlonkDev* d;
  int rc;
  {
    std::lock_guard<std::mutex> lk(pvk->mu);
    if ((rc = plonk_ensure_dev(pvk, device, &d))) return rc;
  }
  // Plan.  Up to `big_from` proofs the batch is cut into up to PLONK_WORKERS contiguous sub-batches, one context and one host thread each, and every sub-batch runs in
  // balanced passes of at most `piece` = 5040 proofs (a sub-batch of 6144 is two passes of 3072): up to there every launch of a pass is ONE wavefront generation and the
  // MSM launches keep their split form, and several such chains of latency-bound launches side by side fill the GPU where one chain of larger launches does not
  // (round 3: 8192 proofs 9.9 -> 8.3 ms, 16 384 15.7 -> 13.1 ms).  From `big_from` proofs the launches are large enough to be throughput-bound on their own and the
  // batch runs as few passes of up to PLONK_MAX_LAUNCH proofs (rounds 4-5; bn254_set_plonk_params has the numbers).
  int workers; size_t per, pass_cap;                                  // sub-batches, proofs per sub-batch, proofs per (equal-sized) pass of a sub-batch
  plonk_plan_for(n, &workers, &per, &pass_cap);
  PlonkLease lease(d, workers);   // waits until that many contexts are free
  for (int w = 0; w < workers; w++) if ((rc = plonk_ensure_ctx(pvk, lease.ctx(w), pass_cap, !resident ? pass_cap * (proof_stride + (d_rows ? 0 : n_public * 32)) : 0))) return rc;
  return plonk_run_workers(lease, workers, per, pass_cap, n, [&](int w, size_t off, size_t m) {
    return plonk_run_device(pvk, d, lease.ctx(w), device, proofs + off * proof_stride, proof_stride, d_rows ? nullptr : public_inputs + off * n_public * 32, n_public, m, status + off,
                            flags, resident, d_rows ? d_rows + off * 64 : nullptr);
  });
}
int plonk_batch_rows(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* d_rows, size_t n, uint8_t* status, int device, unsigned flags,
                     bool resident) {
  return plonk_batch(pvk, proofs, proof_stride, nullptr, 2, n, status, device, flags, resident, d_rows);
}

extern "C" {

int bn254_plonk_verify_batch(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                             size_t n_public, size_t n, uint8_t* status, int device) {
  return bn254_plonk_verify_batch_flags(pvk, proofs, proof_stride, public_inputs, n_public, n, status, device, 0);
}
int bn254_plonk_verify_batch_flags(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                                   size_t n_public, size_t n, uint8_t* status, int device, unsigned flags) {
  int rc = check_batch_args(true, pvk, proofs, proof_stride, public_inputs, n_public, n, status, flags);
  if (rc || n == 0) return rc;
  return plonk_batch(pvk, proofs, proof_stride, public_inputs, n_public, n, status, device, flags, false);
}
// proofs, public inputs and status bytes resident in the memory of `device` (what the bench times: inputs in HBM when the timed region starts)
int bn254_plonk_verify_batch_device(const bn254_plonk_pvk* pvk, const void* d_proofs, size_t proof_stride, const void* d_public_inputs, size_t n_public, size_t n,
                                    void* d_status, int device, void* hip_stream, unsigned flags) {
  int rc = check_batch_args(true, pvk, d_proofs, proof_stride, d_public_inputs, n_public, n, d_status, flags);
  if (rc || n == 0) return rc;
  if ((rc = check_device(device))) return rc;
  // the passes run on the key's own context streams: whatever the caller's stream still has to do to the inputs comes first
  HIPCK(hipStreamSynchronize((hipStream_t)hip_stream));
  return plonk_batch(pvk, (const uint8_t*)d_proofs, proof_stride, (const uint8_t*)d_public_inputs, n_public, n, (uint8_t*)d_status, device, flags, true);
}
// several GPUs of the node: contiguous shards (bn254_shard_plan), one host thread per device through the host-buffer entry -- the PlonK twin of bn254_groth16_verify_batch_multi
int bn254_plonk_verify_batch_multi(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n,
                                   uint8_t* status, uint64_t device_mask, unsigned flags) {
  int prc = check_batch_args(true, pvk, proofs, proof_stride, public_inputs, n_public, n, status, flags);
  if (prc) return prc;
  if (!device_mask) return set_err(BN254_E_BAD_ARG, "bad argument");
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return set_err(BN254_E_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  int devs[64], nsh = 0; size_t los[64], cnts[64];
  if ((prc = bn254_shard_plan(n, device_mask, cnt, devs, los, cnts, &nsh))) return prc;
  if (n == 0) return BN254_OK;
  if (nsh == 1) return plonk_batch(pvk, proofs, proof_stride, public_inputs, n_public, n, status, devs[0], flags, false);
  std::vector<int> rcs((size_t)nsh, BN254_OK); std::vector<std::string> errs((size_t)nsh);
  std::vector<std::thread> th;
  for (int r = 0; r < nsh; r++) {
    th.emplace_back([&, r]() {
      if (!cnts[r]) return;
      rcs[r] = plonk_batch(pvk, proofs + los[r] * proof_stride, proof_stride, public_inputs ? public_inputs + los[r] * n_public * 32 : nullptr, n_public, cnts[r], status + los[r], devs[r], flags, false);
      if (rcs[r]) errs[r] = g_err;   // thread-local in the worker
    });
  }
  for (auto& t : th) t.join();
  for (int r = 0; r < nsh; r++) if (rcs[r]) return set_err(rcs[r], "device " + std::to_string(devs[r]) + ": " + errs[r]);
  return BN254_OK;
}
// Everything a batch of up to n proofs needs on `device`, allocated now: the key's tables, the contexts of the plan such a batch runs under (bn254_set_plonk_params) with
// their row, window-table and workspace buffers, and -- proof_stride > 0: the host-buffer entry will be used -- their pinned staging for records of that stride.  A later
// batch of that size then neither allocates nor frees (growing a context frees its old buffers, and hipFree waits for the whole device).
int bn254_plonk_reserve(const bn254_plonk_pvk* pvk, size_t n, size_t proof_stride, int device) {
  if (!pvk) return set_err(BN254_E_BAD_ARG, "null key");
  if (n == 0) n = 1;
  PlonkDev* d;
  int rc;
  {
    std::lock_guard<std::mutex> lk(pvk->mu);
    if ((rc = plonk_ensure_dev(pvk, device, &d))) return rc;
  }
  int workers; size_t per, pass_cap;
  plonk_plan_for(n, &workers, &per, &pass_cap);
  PlonkLease lease(d, workers);
  const size_t in_bytes = proof_stride ? pass_cap * (proof_stride + (size_t)pvk->key.nb_public * 32) : 0;
  for (int w = 0; w < workers; w++) if ((rc = plonk_ensure_ctx(pvk, lease.ctx(w), pass_cap, in_bytes))) return rc;
  return BN254_OK;
}
// device memory this key holds on `device` right now: its contexts' buffers and the window tables of its points (131 MB for the reference's key); and how many contexts hold any
int bn254_plonk_footprint(const bn254_plonk_pvk* pvk, int device, size_t* bytes, int* contexts) {
  if (!pvk || !bytes) return set_err(BN254_E_BAD_ARG, "bad argument");
  *bytes = 0; if (contexts) *contexts = 0;
  PlonkDev* d = nullptr;
  {
    std::lock_guard<std::mutex> lk(pvk->mu);
    auto it = pvk->dev.find(device);
    if (it != pvk->dev.end()) d = &it->second;
  }
  if (!d) return BN254_OK;
  std::lock_guard<std::mutex> lk(d->pool_mu);
  if (d->fixed_tabs) *bytes += (pvk->fixed_pts.size() / (2 * BN_NL)) * (size_t)MSM_FW_WINDOWS * MSM_FW_ENTRIES * MSM_ENTRY_DWORDS * sizeof(int32_t);
  const int T1 = plonk_stage1_terms(pvk->key), TT = plonk_stage2_terms(pvk->key) + 2;
  const size_t tmax = (size_t)(TT > T1 ? TT : T1);
  for (const PlonkCtx& c : d->ctx) {
    if (!c.cap && !c.in_cap()) continue;
    if (contexts) (*contexts)++;
    *bytes += c.in_cap() + c.cap * (size_t)G16_WS_BYTES_PER_PROOF + c.part_points * 27 * sizeof(int32_t) + c.glv_lanes * (size_t)G1_GLV_TAB_BYTES_PER_LANE +
              c.cap * tmax * (sizeof(MsmTerm) + 1) + c.cap * (16 * sizeof(uint32_t) + 2) + c.cap * bn254_plonk_work_bytes();
  }
  return BN254_OK;
}

void bn254_set_plonk_params(long piece, int workers, long big_from, long big_piece) {
  if (piece >= 0) g_plonk_piece.store(piece < 256 ? 256 : (piece > PLONK_MAX_LAUNCH ? (long)PLONK_MAX_LAUNCH : piece));
  if (workers >= 0) g_plonk_workers.store(workers < 1 ? 1 : (workers > PLONK_WORKERS ? PLONK_WORKERS : workers));
  if (big_from >= 0) g_plonk_big_from.store(big_from);      // 0: the measured default plan
  if (big_piece >= 0) g_plonk_big_piece.store(big_piece < 256 ? 256 : (big_piece > PLONK_MAX_LAUNCH ? (long)PLONK_MAX_LAUNCH : big_piece));
}

// the pass size from which BN254_FLAG_RLC is honoured, on one key and over a list (initial value: BN254_PLONK_RLC_MIN, default 8192): a group is 64 proofs, so never below 64
void bn254_set_plonk_rlc_params(long min_pass) {
  if (min_pass >= 0) g_plonk_rlc_min.store(min_pass < 64 ? 64 : min_pass);
}

int bn254_plonk_verify(const uint8_t* proof, size_t proof_len, const uint8_t* vk, size_t vk_len, const uint8_t* public_inputs,
                       size_t n_public, uint8_t* status) {
  if (!proof || !vk || !status) return set_err(BN254_E_BAD_ARG, "bad argument");
  std::shared_ptr<bn254_plonk_pvk> pvk = plonk_key_cache().find(vk, vk_len, 0);
  if (!pvk) {
    bn254_plonk_pvk* raw = nullptr;
    int rc = bn254_plonk_vk_prepare(vk, vk_len, &raw);
    if (rc == BN254_E_VK) {
      // the proof is loaded before the key (lib.rs:70 before :71): its loader error (short buffer, coordinate >= p, off the curve; plonk/converter.rs:121-178) wins
      // over the key's.  Host work for this one proof: no kernel can run without a key
      PlonkProof pr;
      const int ps = parse_plonk_proof(pr, proof, proof_len);
      *status = ps == PL_OK ? (uint8_t)BN254_ERR_MALFORMED : (uint8_t)ps;
      return BN254_OK;
    }
    if (rc) return rc;
    pvk = plonk_key_cache().insert(vk, vk_len, 0, raw);
  }
  return bn254_plonk_verify_batch(pvk.get(), proof, proof_len, public_inputs, n_public, 1, status, 0);
}

}  // extern "C"
