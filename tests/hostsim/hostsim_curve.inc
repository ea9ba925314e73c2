// included inside extern "C" of hostsim.cpp when HS_WITH_CURVE is defined
static G1Aff g1_in(const uint8_t* b) { G1Aff r; r.x = fp_in(b, 0); r.y = fp_in(b + 32, 0); return r; }
static bool all_zero(const uint8_t* b, int n) { for (int i = 0; i < n; i++) if (b[i]) return false; return true; }
static void g1_out(uint8_t* o, const G1Proj& p) {
  if (g1_is_identity(p)) { memset(o, 0, 64); return; }
  G1Aff a = g1_to_affine(p); fp_out(o, a.x); fp_out(o + 32, a.y);
}
static G2Aff g2_in(const uint8_t* b) {  // gnark order x.c1 x.c0 y.c1 y.c0
  G2Aff r; r.x.c1 = fp_in(b, 0); r.x.c0 = fp_in(b + 32, 0); r.y.c1 = fp_in(b + 64, 0); r.y.c0 = fp_in(b + 96, 0); return r;
}
// op 0: mixed add (p may be all-zero = identity; q finite), 1: dbl, 2: general add (either may be identity), 3: on_curve -> o[0]
void hs_g1_op(int op, uint8_t* o, const uint8_t* p, const uint8_t* q) {
  G1Proj P = all_zero(p, 64) ? g1_identity() : g1_from_affine(g1_in(p));
  G1Proj R = g1_identity();
  switch (op) {
    case 0: R = g1_add_mixed(P, g1_in(q)); break;
    case 1: R = g1_dbl(P); break;
    case 2: R = g1_add(P, all_zero(q, 64) ? g1_identity() : g1_from_affine(g1_in(q))); break;
    case 3: memset(o, 0, 64); o[0] = g1_on_curve(g1_in(p)) ? 1 : 0; return;
  }
  g1_out(o, R);
}
// chained complete mixed additions starting from the identity: sum of n affine points (exercises non-trivial Z)
void hs_g1_sum(uint8_t* o, const uint8_t* pts, int n) {
  G1Proj acc = g1_identity();
  for (int i = 0; i < n; i++) acc = g1_add_mixed(acc, g1_in(pts + 64 * i));
  g1_out(o, acc);
}
int hs_g2_on_curve(const uint8_t* p) { return g2_on_curve(g2_in(p)) ? 1 : 0; }
int hs_g2_in_subgroup(const uint8_t* p) { return g2_in_subgroup(g2_in(p)) ? 1 : 0; }
// Miller loop with one variable pair and nf (0..2) fixed pairs whose G2 arguments get precomputed tables
int hs_miller(uint8_t* o, const uint8_t* pa, const uint8_t* qb, int nf, const uint8_t* pf, const uint8_t* qf) {
  static FixedLine tab[2][BN_ATE_STEPS];
  G1Aff pfs[2]; const FixedLine* tabs[2] = {tab[0], tab[1]};
  for (int k = 0; k < nf; k++) { pfs[k] = g1_in(pf + 64 * k); if (!fixed_line_table(tab[k], g2_in(qf + 128 * k))) return 0; }
  Fp12 f = nf == 0 ? miller_loop<0>(g1_in(pa), g2_in(qb), pfs, tabs) : nf == 1 ? miller_loop<1>(g1_in(pa), g2_in(qb), pfs, tabs)
                                                                              : miller_loop<2>(g1_in(pa), g2_in(qb), pfs, tabs);
  fp12_out(o, f);
  return 1;
}
void hs_final_exp(uint8_t* o, const uint8_t* f) { fp12_out(o, final_exponentiation(fp12_in(f, 0))); }

// ---- the workspace "VM" (bn254_vm.h) on plain host arrays: same operation sequence as the GPU kernels ----------------------------
struct HostWs {
  Fp el[VE_COUNT];
  Fp2 parked[4];
  void park(int slot, const Fp2& a) { parked[slot] = a; }
  Fp2 unpark(int slot) { return parked[slot]; }
  Fp ld(int e) { return el[e]; }
  void st(int e, const Fp& a) { el[e] = a; }
};
struct HostOps {
  HostWs& w; const FixedLine* tab[2]; bool inf;
  int uni(int x) { return x; }
  void f12_sqr(int e) { vm_f12_sqr(w, e); }
  void miller_dbl_var(int et, int e, int ep) { vm_miller_dbl_var(w, et, e, ep); }
  void miller_step(bool do_sqr, int kind, int s, int et, int eb, int e, int epa, int ep0, int ep1) {
    if (do_sqr) vm_miller_step<true>(w, kind, et, eb, e, epa, tab[0][s], ep0, inf, tab[1][s], ep1, false);
    else vm_miller_step<false>(w, kind, et, eb, e, epa, tab[0][s], ep0, inf, tab[1][s], ep1, false);
  }
  struct Lines { const FixedLine* const* tab; const FixedLine& get(int t, int s) const { return tab[t][s]; } };
  struct Kinds { int get(int s) const { return miller_step_kind(s); } };
  void miller_run(int s_begin, int s_end, int et, int eb, int e, int epa, int ep0, int ep1) {
    Lines lines{tab};
    vm_miller_run(w, lines, Kinds{}, s_begin, s_end, et, eb, e, epa, ep0, inf, ep1, false);
  }
  void miller_sqr_dbl_var(int et, int e, int ep) { vm_miller_sqr_dbl_var(w, et, e, ep); }
  void miller_add_var(int et, int eb, int which, int e, int ep) { vm_miller_add_var(w, et, eb, which, e, ep); }
  void f12_mul_line_fixed(int e, int t, int s, int ep) { vm_f12_mul_line_fixed(w, e, tab[t][s], ep, t == 0 && inf); }
  void f12_mul_line_fixed2(int e, int s, int ep0, int ep1) { vm_f12_mul_line_fixed2(w, e, tab[0][s], ep0, inf, tab[1][s], ep1, false); }
  void f12_mul(int d, int a, int b, bool conj_b = false) { vm_f12_mul(w, d, a, b, conj_b); }
  void f12_copy(int d, int a) { vm_f12_copy(w, d, a); }
  void f12_cyclo_sqr(int d, int a) { vm_f12_cyclo_sqr(w, d, a); }
  void f12_cyclo_sqr_n(int d, int a, int count) { vm_f12_cyclo_sqr_n(w, d, a, count); }
  void f12_conj(int d, int a) { vm_f12_conj(w, d, a); }
  void f12_frob(int d, int a, int j) { vm_f12_frob(w, d, a, j); }
  void f12_inv(int d, int a) { vm_f12_inv(w, d, a); }
};
static void put_g1(HostWs& w, int e, const G1Aff& p) { w.el[e] = p.x; w.el[e + 1] = p.y; }
// the latency-mode program of bn254_launch_g16 (small batches): three separate Miller chains -- variable pair on VE_F, the two
// table-driven pairs on VE_S1 / VE_S2 -- multiplied together before the final exponentiation.  Same output as hs_vm_pairing3.
int hs_vm_pairing3_split(uint8_t* o, const uint8_t* pa, const uint8_t* qb, const uint8_t* pl, const uint8_t* qg, const uint8_t* pc, const uint8_t* qd, int l_inf) {
  static FixedLine tg[BN_ATE_STEPS], td[BN_ATE_STEPS];
  if (!fixed_line_table(tg, g2_in(qg)) || !fixed_line_table(td, g2_in(qd))) return 0;
  static HostWs w;
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
  put_g1(w, VE_AX, g1_in(pa)); put_g1(w, VE_CX, g1_in(pc));
  G1Aff L = g1_in(pl);
  if (l_inf) { L.x = fp_zero(); L.y = fp_one(); }
  put_g1(w, VE_LX, L);
  G2Aff B = g2_in(qb);
  w.el[VE_B] = B.x.c0; w.el[VE_B + 1] = B.x.c1; w.el[VE_B + 2] = B.y.c0; w.el[VE_B + 3] = B.y.c1;
  w.el[VE_F] = fp_one();
  w.el[VE_T] = B.x.c0; w.el[VE_T + 1] = B.x.c1; w.el[VE_T + 2] = B.y.c0; w.el[VE_T + 3] = B.y.c1; w.el[VE_T + 4] = fp_one();
  HostOps ops{w, {tg, td}, l_inf != 0};
  ops.f12_copy(VE_S1, VE_F); ops.f12_copy(VE_S2, VE_F);
  for (int s = 0; s < BN_ATE_STEPS; s++) {
    int kind = miller_step_kind(s);
    if (kind == 0) { if (s != 0) ops.miller_sqr_dbl_var(VE_T, VE_F, VE_AX); else ops.miller_dbl_var(VE_T, VE_F, VE_AX); }
    else ops.miller_add_var(VE_T, VE_B, kind - 1, VE_F, VE_AX);
    if (kind == 0 && s != 0) { ops.f12_sqr(VE_S1); ops.f12_sqr(VE_S2); }
    ops.f12_mul_line_fixed(VE_S1, 0, s, VE_LX);
    ops.f12_mul_line_fixed(VE_S2, 1, s, VE_CX);
  }
  ops.f12_mul(VE_F, VE_F, VE_S1); ops.f12_mul(VE_F, VE_F, VE_S2);
  vm_final_exp_program(ops);
  static const int korder[6] = {0, 2, 4, 1, 3, 5};
  for (int t = 0; t < 6; t++) { fp_out(o + 64 * t, w.el[VE_S0 + 2 * korder[t]]); fp_out(o + 64 * t + 32, w.el[VE_S0 + 2 * korder[t] + 1]); }
  return 1;
}
// the product's r-torsion test: Miller program on (pa, qb) without fixed pairs, then the ate relation on the final T
int hs_vm_g2_ate_check(const uint8_t* pa, const uint8_t* qb) {
  static HostWs w;
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
  put_g1(w, VE_AX, g1_in(pa));
  G2Aff B = g2_in(qb);
  w.el[VE_B] = B.x.c0; w.el[VE_B + 1] = B.x.c1; w.el[VE_B + 2] = B.y.c0; w.el[VE_B + 3] = B.y.c1;
  w.el[VE_F] = fp_one();
  w.el[VE_T] = B.x.c0; w.el[VE_T + 1] = B.x.c1; w.el[VE_T + 2] = B.y.c0; w.el[VE_T + 3] = B.y.c1; w.el[VE_T + 4] = fp_one();
  uint8_t kinds[BN_ATE_STEPS];
  for (int s = 0; s < BN_ATE_STEPS; s++) kinds[s] = (uint8_t)miller_step_kind(s);
  HostOps ops{w, {nullptr, nullptr}, false};
  vm_miller_program(ops, kinds, false);
  return vm_g2_ate_check(w, VE_T, VE_B) ? 1 : 0;
}
// e(pa, qb) * e(pl, qg) * e(pc, qd) through the VM programs; l_inf: treat pl as the identity.  Output in tower byte order.
int hs_vm_pairing3(uint8_t* o, const uint8_t* pa, const uint8_t* qb, const uint8_t* pl, const uint8_t* qg, const uint8_t* pc, const uint8_t* qd, int l_inf) {
  static FixedLine tg[BN_ATE_STEPS], td[BN_ATE_STEPS];
  if (!fixed_line_table(tg, g2_in(qg)) || !fixed_line_table(td, g2_in(qd))) return 0;
  static HostWs w;
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
  put_g1(w, VE_AX, g1_in(pa)); put_g1(w, VE_CX, g1_in(pc));
  G1Aff L = g1_in(pl);
  if (l_inf & 1) { L.x = fp_zero(); L.y = fp_one(); }
  put_g1(w, VE_LX, L);
  G2Aff B = g2_in(qb);
  w.el[VE_B] = B.x.c0; w.el[VE_B + 1] = B.x.c1; w.el[VE_B + 2] = B.y.c0; w.el[VE_B + 3] = B.y.c1;
  w.el[VE_F] = fp_one();
  w.el[VE_T] = B.x.c0; w.el[VE_T + 1] = B.x.c1; w.el[VE_T + 2] = B.y.c0; w.el[VE_T + 3] = B.y.c1; w.el[VE_T + 4] = fp_one();
  uint8_t kinds[BN_ATE_STEPS];
  for (int s = 0; s < BN_ATE_STEPS; s++) kinds[s] = (uint8_t)miller_step_kind(s);
  HostOps ops{w, {tg, td}, (l_inf & 1) != 0};
  if (l_inf & 2) vm_miller_program_runs(ops, (l_inf >> 2) ? (l_inf >> 2) : BN_ATE_STEPS);   // bit 1: the run form of the Miller loop, l_inf >> 2 steps per operation (0: all)
  else vm_miller_program(ops, kinds);
  vm_final_exp_program(ops);
  // k-order -> tower order: c0 = (k0, k2, k4), c1 = (k1, k3, k5)
  static const int korder[6] = {0, 2, 4, 1, 3, 5};
  for (int t = 0; t < 6; t++) { fp_out(o + 64 * t, w.el[VE_S0 + 2 * korder[t]]); fp_out(o + 64 * t + 32, w.el[VE_S0 + 2 * korder[t] + 1]); }
  return 1;
}

// e(p0, q0) * e(p1, q1) through the two-fixed-pair run (bn254_vm.h::vm_miller_run_fixed2, per_run steps per operation; 0: the whole loop) + the final
// exponentiation program: what the lane path of PlonK's KZG check runs.  inf bit 0 / 1: treat p0 / p1 as the identity.
int hs_vm_pairing2_fixed(uint8_t* o, const uint8_t* p0, const uint8_t* q0, const uint8_t* p1, const uint8_t* q1, int inf, int per_run) {
  static FixedLine t0[BN_ATE_STEPS], t1[BN_ATE_STEPS];
  if (!fixed_line_table(t0, g2_in(q0)) || !fixed_line_table(t1, g2_in(q1))) return 0;
  static HostWs w;
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
  G1Aff P0 = g1_in(p0), P1 = g1_in(p1);
  if (inf & 1) { P0.x = fp_zero(); P0.y = fp_one(); }
  if (inf & 2) { P1.x = fp_zero(); P1.y = fp_one(); }
  put_g1(w, VE_LX, P0); put_g1(w, VE_CX, P1);
  w.el[VE_F] = fp_one();
  const FixedLine* tabs[2] = {t0, t1};
  HostOps::Lines lines{tabs};
  if (per_run <= 0) per_run = BN_ATE_STEPS;
  for (int s = 0; s < BN_ATE_STEPS; s += per_run)
    vm_miller_run_fixed2(w, lines, HostOps::Kinds{}, s, s + per_run < BN_ATE_STEPS ? s + per_run : BN_ATE_STEPS, VE_F, VE_LX, (inf & 1) != 0, VE_CX, (inf & 2) != 0);
  HostOps ops{w, {t0, t1}, false};
  vm_final_exp_program(ops);
  static const int korder[6] = {0, 2, 4, 1, 3, 5};
  for (int t = 0; t < 6; t++) { fp_out(o + 64 * t, w.el[VE_S0 + 2 * korder[t]]); fp_out(o + 64 * t + 32, w.el[VE_S0 + 2 * korder[t] + 1]); }
  return 1;
}

// ---- RLC batch mode (bn254_rlc.h) on host arrays: the whole group pipeline for n proofs forming groups per rlc_plan(n, log2_group) -------------
// proofs: n x 256 B (A | B | C, gnark uncompressed), inputs: n x n_public x 32 B big-endian, alpha: 64 B (negated here), ks: (n_public + 1) x 64 B,
// qg / qd / qb: the key-side G2 arguments g', d', b' (128 B each).  key44: ChaCha key (32 B) + nonce (12 B).  out_groups[g] = 1 if group g's
// product is one; out_group_of[i] = group of proof i; bad_mask bit i: treat proof i as a loader error (neutral lane).  Returns the group count.
// weight_mode 0: proof i draws ChaCha20 counter i, as k_rlc_scale does; 1 (this stand-in's own, for tests/test_rlc_forgery_cpu.py): every proof draws counter 0,
// so all weights are equal -- the defect a pair of proofs with opposite errors passes under.
struct HostWs2 {
  HostWs *lo, *hi;
  void park(int slot, const Fp2& a) { lo->park(slot, a); }
  Fp2 unpark(int slot) { return lo->unpark(slot); }
  Fp ld(int e) { return e >= RLC_HI ? hi->el[e - RLC_HI] : lo->el[e]; }
  void st(int e, const Fp& a) { lo->el[e] = a; }
};
static G1Aff hs_small_multiple(const G1Aff& base, int wi, int d) {  // (d + 1) * 2^(MSM_FW_BITS wi) * base: what entry d of window wi of the base's table holds (bn254_fw.h)
  G1Proj p = g1_from_affine(base);
  for (int i = 0; i < MSM_FW_BITS * wi; i++) p = g1_dbl(p);
  G1Aff pa = g1_to_affine(p);
  G1Proj acc = g1_identity();
  for (int b = MSM_FW_BITS; b >= 0; b--) { acc = g1_dbl(acc); if (((d + 1) >> b) & 1) acc = g1_add_mixed(acc, pa); }
  return g1_to_affine(acc);
}
// the accessor of the shared-accumulator Miller loop on host arrays: proof q of lane j is ws[j + q m]
struct HostWsM {
  HostWs* ws; int j, m, n, cur;
  void sel(int q) { cur = j + q * m; }
  void park(int slot, const Fp2& a) { ws[j].park(slot, a); }
  Fp2 unpark(int slot) { return ws[j].unpark(slot); }
  Fp ld(int e) { return cur < n ? ws[cur].el[e] : fp_zero(); }
  void st(int e, const Fp& a) { if (cur < n) ws[cur].el[e] = a; }
  Fp ld0(int e) { return ws[j].el[e]; }
  void st0(int e, const Fp& a) { ws[j].el[e] = a; }
};
int hs_rlc_pipeline(int n, const uint8_t* proofs, const uint8_t* inputs, int n_public, const uint8_t* alpha, const uint8_t* ks,
                    const uint8_t* qg, const uint8_t* qd, const uint8_t* qb, const uint8_t* key44, int log2_group, uint32_t bad_mask,
                    uint8_t* out_groups, uint32_t* out_group_of, int log2_share, int weight_mode) {
  static FixedLine tg[BN_ATE_STEPS], td[BN_ATE_STEPS], tb[BN_ATE_STEPS];
  if (!fixed_line_table(tg, g2_in(qg)) || !fixed_line_table(td, g2_in(qd)) || !fixed_line_table(tb, g2_in(qb))) return -1;
  ChaChaKey key;
  for (int i = 0; i < 8; i++) key.k[i] = (uint32_t)key44[4 * i] | (uint32_t)key44[4 * i + 1] << 8 | (uint32_t)key44[4 * i + 2] << 16 | (uint32_t)key44[4 * i + 3] << 24;
  for (int i = 0; i < 3; i++) key.nonce[i] = (uint32_t)key44[32 + 4 * i] | (uint32_t)key44[33 + 4 * i] << 8 | (uint32_t)key44[34 + 4 * i] << 16 | (uint32_t)key44[35 + 4 * i] << 24;
  HostWs* ws = new HostWs[n];
  uint8_t kinds[BN_ATE_STEPS];
  for (int s = 0; s < BN_ATE_STEPS; s++) kinds[s] = (uint8_t)miller_step_kind(s);
  for (int i = 0; i < n; i++) {
    HostWs& w = ws[i];
    for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
    const uint8_t* p = proofs + 256 * i;
    put_g1(w, VE_AX, g1_in(p)); put_g1(w, VE_CX, g1_in(p + 192));
    G2Aff B = g2_in(p + 64);
    w.el[VE_B] = B.x.c0; w.el[VE_B + 1] = B.x.c1; w.el[VE_B + 2] = B.y.c0; w.el[VE_B + 3] = B.y.c1;
    w.el[VE_F] = fp_one();
    w.el[VE_T] = B.x.c0; w.el[VE_T + 1] = B.x.c1; w.el[VE_T + 2] = B.y.c0; w.el[VE_T + 3] = B.y.c1; w.el[VE_T + 4] = fp_one();
    uint32_t r[4];
    chacha20_block4(r, key, weight_mode == 1 ? 0u : (uint32_t)i);
    const uint8_t* in = inputs + (size_t)i * n_public * 32;
    vm_rlc_scale(w, r, n_public, [&](int j, uint32_t* o) { words_from_be(o, in + 32 * j); });
    if (log2_share == 0) {
      HostOps ops{w, {nullptr, nullptr}, false};
      vm_miller_program(ops, kinds, false);
      bool ok = vm_g2_ate_check(w, VE_T, VE_B) && !((bad_mask >> i) & 1);
      if (!ok) vm_rlc_neutral(w, n_public);
    }
  }
  RlcPlan plan = rlc_plan((uint32_t)n, log2_group, log2_share);
  if (log2_share > 0) {
    // shared accumulators: lane j < m walks proofs j, j + m, ...; loader errors (bad_mask) are known before the loop and masked out of f
    const int share = 1 << log2_share, m = (int)plan.lanes;
    for (int j = 0; j < m; j++) {
      ws[j].el[VE_F] = fp_one();
      for (int e = 1; e < 12; e++) ws[j].el[VE_F + e] = fp_zero();
      uint32_t dead = 0;
      for (int q = 0; q < share; q++) if (j + q * m >= n || ((bad_mask >> (j + q * m)) & 1)) dead |= 1u << q;
      HostWsM wm{ws, j, m, n, j};
      for (int s = 0; s < BN_ATE_STEPS; s++) {
        if (kinds[s] == 0 && s != 0) vm_miller_var_multi<true>(wm, kinds[s], share, dead);
        else vm_miller_var_multi<false>(wm, kinds[s], share, dead);
      }
    }
    for (int i = 0; i < n; i++) {
      bool ok = vm_g2_ate_check(ws[i], VE_T, VE_B) && !((bad_mask >> i) & 1);
      if (!ok) vm_rlc_neutral(ws[i], n_public, false);
    }
  }
  uint32_t cur = (uint32_t)n;
  for (int k = 0; k < plan.rounds; k++) {
    uint32_t half = plan.half[k];
    for (uint32_t j = 0; j + half < cur; j++) { HostWs2 w2{&ws[j], &ws[j + half]}; vm_rlc_fold(w2, n_public, k >= plan.pre); }
    cur = half;
  }
  for (int i = 0; i < n; i++) out_group_of[i] = rlc_group_of((uint32_t)i, plan);
  G1Aff na = g1_neg(g1_in(alpha));
  Fp12 one = fp12_one();
  for (uint32_t g = 0; g < plan.groups; g++) {
    HostWs& w = ws[g];
    int flags = vm_rlc_group_points(w, n_public, [&](int b, int wi, int d) { return hs_small_multiple(b == 0 ? na : g1_in(ks + 64 * (b - 1)), wi, d); });
    for (int s = 0; s < BN_ATE_STEPS; s++) {
      if (kinds[s] == 0 && s != 0) vm_miller_step_fixed3<true>(w, RLC_ACC, tg[s], VE_LX, (flags & 1) != 0, td[s], VE_CX, (flags & 2) != 0, tb[s], VE_AX, (flags & 4) != 0);
      else vm_miller_step_fixed3<false>(w, RLC_ACC, tg[s], VE_LX, (flags & 1) != 0, td[s], VE_CX, (flags & 2) != 0, tb[s], VE_AX, (flags & 4) != 0);
    }
    vm_f12_mul(w, VE_F, VE_F, RLC_ACC);
    HostOps ops{w, {nullptr, nullptr}, false};
    vm_final_exp_program(ops);
    Fp12 res;
    K0(res) = vld2(w, VE_S0); K1(res) = vld2(w, VE_S0 + 2); K2(res) = vld2(w, VE_S0 + 4); K3(res) = vld2(w, VE_S0 + 6); K4(res) = vld2(w, VE_S0 + 8); K5(res) = vld2(w, VE_S0 + 10);
    out_groups[g] = fp12_eq(res, one) ? 1 : 0;
  }
  delete[] ws;
  return (int)plan.groups;
}
// probes of the Fr arithmetic and the weight generator
void hs_fr8_mul_plain(uint8_t* o32, const uint8_t* x32, const uint8_t* k32) {
  Fr8 x, k; words_from_be(x.w, x32); words_from_be(k.w, k32);
  Fr8 r = fr8_mul_plain(x, k);
  words_to_be(o32, r.w);
}
void hs_fr8_add(uint8_t* o32, const uint8_t* x32, const uint8_t* k32) {
  Fr8 x, k; words_from_be(x.w, x32); words_from_be(k.w, k32);
  Fr8 r = fr8_add(x, k);
  words_to_be(o32, r.w);
}
void hs_chacha_block4(uint32_t* out4, const uint8_t* key44, uint32_t counter) {
  ChaChaKey key;
  for (int i = 0; i < 8; i++) key.k[i] = (uint32_t)key44[4 * i] | (uint32_t)key44[4 * i + 1] << 8 | (uint32_t)key44[4 * i + 2] << 16 | (uint32_t)key44[4 * i + 3] << 24;
  for (int i = 0; i < 3; i++) key.nonce[i] = (uint32_t)key44[32 + 4 * i] | (uint32_t)key44[33 + 4 * i] << 8 | (uint32_t)key44[34 + 4 * i] << 16 | (uint32_t)key44[35 + 4 * i] << 24;
  chacha20_block4(out4, key, counter);
}
// (+-k1 +- k2 lambda) P with 128-bit halves by the joint two-bit-window form (bn254_rlc.h::g1_mul_glv_w2, table in a host array) and, for comparison,
// by the one-bit form (g1_mul_glv_w): k32_be = k2 (16 bytes, big-endian) | k1 (16 bytes); signs: bit 0 k1 negative, bit 1 k2 negative
struct HsGlvTab {
  G1Proj own[16]; G1Proj* t;                            // a table of its own, or slot j of a caller's array (joint rows: one table per term)
  HsGlvTab() : t(own) {}
  explicit HsGlvTab(G1Proj* store) : t(store) {}
  HsGlvTab(const HsGlvTab& o) : t(o.t == o.own ? own : o.t) { if (t == own) for (int i = 0; i < 16; i++) own[i] = o.own[i]; }
  void put(int i, const G1Proj& p) { t[i] = p; t[i].x = fp_reduce(t[i].x); t[i].y = fp_reduce(t[i].y); t[i].z = fp_reduce(t[i].z); }
  G1Proj get(uint32_t i) const { return t[i]; }
  void fence() {}
  HsGlvTab slot(int j) const { return HsGlvTab(t + 16 * j); }
};
void hs_g1_mul_glv_w2(uint8_t* o64_w2, uint8_t* o64_w1, const uint8_t* p64, const uint8_t* k32_be, int signs) {
  uint32_t k1[4], k2[4];
  for (int i = 0; i < 4; i++) {
    const uint8_t* q2 = k32_be + 4 * (3 - i); const uint8_t* q1 = k32_be + 16 + 4 * (3 - i);
    k2[i] = (uint32_t)q2[0] << 24 | (uint32_t)q2[1] << 16 | (uint32_t)q2[2] << 8 | q2[3];
    k1[i] = (uint32_t)q1[0] << 24 | (uint32_t)q1[1] << 16 | (uint32_t)q1[2] << 8 | q1[3];
  }
  HsGlvTab tab;
  g1_out(o64_w2, g1_mul_glv_w2<4>(g1_in(p64), k1, (signs & 1) != 0, k2, (signs & 2) != 0, tab));
  g1_out(o64_w1, g1_mul_glv_w<4>(g1_in(p64), k1, (signs & 1) != 0, k2, (signs & 2) != 0));
}
// k16_be: k2 (8 bytes, big-endian) | k1 (8 bytes): the point (k1 + k2 lambda) P and the weight as a 32-byte big-endian Fr value
void hs_g1_mul_glv(uint8_t* o64, uint8_t* weight32, const uint8_t* p64, const uint8_t* k16_be) {
  uint32_t k[4];
  for (int i = 0; i < 4; i++) { const uint8_t* q = k16_be + 4 * (3 - i); k[i] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3]; }
  g1_out(o64, g1_mul_glv(g1_in(p64), k));
  Fr8 wv = rlc_weight(k);
  words_to_be(weight32, wv.w);
}

// ---- the MSM rows of the PlonK path (bn254_msm.h) on the host: plan the launch, evaluate EVERY row as a lane of k_g1_msm_rows would, add the rows of each sum.
// shape: n_sums | per sum: n_var, n_unit, n_fixed | per sum: var terms, unit terms, fixed terms, fixed tables (ints).
// terms: n_terms records of 129 bytes: point (64, big-endian x | y) | k1 (16, big-endian) | k2 (16) | scalar (32, LITTLE-endian bytes: the 8 canonical words) | flag byte
//        (bit 0: identity, bits 1 / 2: signs of k1 / k2, or the sign of a unit term).  bases: the key points the fixed tables are built from (64 bytes each).
// out: per sum 64 bytes (zero = identity); info: rows, variable rows, longest row (planner units), rows of sum 0, rows of sum 1.  Returns 0 if the shape cannot be planned.
struct HsMsmIO {
  const uint8_t* terms; const uint8_t* bases;
  void term(int t, G1Aff& P, uint32_t k1[4], uint32_t k2[4], uint32_t& fl) const {
    const uint8_t* e = terms + 129 * (size_t)t;
    if (all_zero(e, 64)) { P.x = fp_zero(); P.y = fp_zero(); } else P = g1_in(e);
    for (int i = 0; i < 4; i++) {
      const uint8_t* q1 = e + 64 + 4 * (3 - i); const uint8_t* q2 = e + 80 + 4 * (3 - i);
      k1[i] = (uint32_t)q1[0] << 24 | (uint32_t)q1[1] << 16 | (uint32_t)q1[2] << 8 | q1[3];
      k2[i] = (uint32_t)q2[0] << 24 | (uint32_t)q2[1] << 16 | (uint32_t)q2[2] << 8 | q2[3];
    }
    fl = e[128];
  }
  uint32_t kword(int t, int half, int w) const {
    const uint8_t* q = terms + 129 * (size_t)t + 64 + 16 * half + 4 * (3 - w);
    return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
  }
  // digit w (MSM_FW_BITS bits) of the scalar whose 32 bytes sit little-endian at terms[.. + 96]
  uint32_t scalar_digit(int t, int w) const {
    const uint8_t* q = terms + 129 * (size_t)t + 96;
    uint32_t v = 0;
    for (int b = 0; b < MSM_FW_BITS; b++) { const int bit = MSM_FW_BITS * w + b; if (bit < 256 && ((q[bit >> 3] >> (bit & 7)) & 1)) v |= 1u << b; }
    return v;
  }
  // (d + 1) 2^(MSM_FW_BITS w) base, by plain double-and-add; 2^(MSM_FW_BITS w) base is kept per base (the tests run hundreds of items against the same bases)
  // The memo is process-wide state shared by every HsMsmIO and is NOT thread-safe: the callers are single-threaded ctypes tests.  It only saves doublings:
  // an entry is a function of the base's bytes alone, so clearing it or missing it changes no value.
  const G1Proj& window_base(int tab, int w) const {
    static std::map<std::array<uint8_t, 64>, std::vector<G1Proj>> memo;
    std::array<uint8_t, 64> key;
    memcpy(key.data(), bases + 64 * (size_t)tab, 64);
    auto it = memo.find(key);
    if (it == memo.end()) {
      if (memo.size() >= 64) memo.clear();
      std::vector<G1Proj> bw(MSM_FW_WINDOWS);
      G1Proj b = g1_from_affine(g1_in(key.data()));
      for (int k = 0; k < MSM_FW_WINDOWS; k++) { bw[k] = b; for (int i = 0; i < MSM_FW_BITS; i++) b = g1_dbl(b); }
      it = memo.emplace(key, bw).first;
    }
    return it->second[w];
  }
  G1Aff entry(int tab, int w, uint32_t d) const {
    const G1Proj bw = window_base(tab, w);
    G1Proj acc = g1_identity();
    for (int bit = MSM_FW_BITS; bit >= 0; bit--) { acc = g1_dbl(acc); if (((d + 1) >> bit) & 1) acc = g1_add(acc, bw); }
    G1Aff r = g1_to_affine(acc);
    r.x = fp_reduce(r.x); r.y = fp_reduce(r.y);
    return r;
  }
};
// A row as it travels from k_g1_msm_rows to k_g1_sum_affine: msm_rows_body stores the digits of the accumulator as they are, and the sum kernel declares
// BN_SETB(t, 3.0, 0.5) on what it loads.  The row must be inside that declaration by the tracker's own account; then it carries the DECLARED bound, so that the
// addition the device performs is the one the tracker checks.
static G1Proj hs_row_through_memory(G1Proj row) {
  Fp* c[3] = {&row.x, &row.y, &row.z};
  for (int k = 0; k < 3; k++) {
    if (BN_VB(*c[k]) > 3.0 || BN_LBD(*c[k]) > 0.5) fp_dbg_fail("an MSM row exceeds the bound k_g1_sum_affine declares for it", BN_VB(*c[k]));
    BN_SETB(*c[k], 3.0, 0.5);
  }
  return row;
}
int hs_msm_rows_joint(uint8_t* out, int* info, const int* shape, const uint8_t* terms, const uint8_t* bases, unsigned n_pad, unsigned lane_budget, int joint_g);
int hs_msm_rows(uint8_t* out, int* info, const int* shape, const uint8_t* terms, const uint8_t* bases, unsigned n_pad, unsigned lane_budget) {
  return hs_msm_rows_joint(out, info, shape, terms, bases, n_pad, lane_budget, 0);
}
// joint_g > 1: unsplit launches walk up to joint_g variable terms of a sum in one joint row (msm_plan_build)
int hs_msm_rows_joint(uint8_t* out, int* info, const int* shape, const uint8_t* terms, const uint8_t* bases, unsigned n_pad, unsigned lane_budget, int joint_g) {
  MsmShape sh; memset(&sh, 0, sizeof sh);
  const int* q = shape;
  sh.n_sums = *q++;
  for (int s = 0; s < sh.n_sums; s++) { sh.n_var[s] = *q++; sh.n_unit[s] = *q++; sh.n_fixed[s] = *q++; }
  for (int s = 0; s < sh.n_sums; s++) {
    for (int i = 0; i < sh.n_var[s]; i++) sh.var_term[s][i] = (int8_t)*q++;
    for (int i = 0; i < sh.n_unit[s]; i++) sh.unit_term[s][i] = (int8_t)*q++;
    for (int i = 0; i < sh.n_fixed[s]; i++) sh.fixed_term[s][i] = (int8_t)*q++;
    for (int i = 0; i < sh.n_fixed[s]; i++) sh.fixed_tab[s][i] = (int8_t)*q++;
  }
  MsmPlan plan;
  if (!msm_plan_build(plan, sh, n_pad, lane_budget, 0, joint_g)) return 0;
  HsMsmIO io{terms, bases};
  for (int s = 0; s < sh.n_sums; s++) {
    G1Proj sum = g1_identity();
    for (int r = plan.first[s]; r < plan.first[s] + plan.count[s]; r++) {
      static G1Proj store[16 * MSM_MAX_JOINT];
      HsGlvTab tab(store);
      G1Proj row = msm_row_eval(plan, r, io, tab);
      sum = g1_add(sum, hs_row_through_memory(row));
    }
    g1_out(out + 64 * s, sum);
  }
  info[0] = plan.n_rows; info[1] = plan.n_var_rows; info[2] = msm_plan_chain(plan); info[3] = plan.count[0]; info[4] = plan.count[1];
  return 1;
}
// k_g1_sum_affine on rows the caller places as raw digits (27 int32 per row: X, Y, Z as given, declared at the kernel's bound for a loaded row): lane q of lpi
// (1 or 4) adds rows q, q + lpi, ..., then the butterfly steps of the kernel; out: the affine sum (zero = identity).  Returns 0 on a bad argument.
int hs_g1_sum_rows_raw(uint8_t* out, const int32_t* rows, int count, int lpi) {
  if (count < 1 || count > MSM_MAX_ROWS || (lpi != 1 && lpi != 4)) return 0;
  G1Proj L[4];
  for (int q = 0; q < lpi; q++) {
    L[q] = g1_identity();
    for (int cc = q; cc < count; cc += lpi) {
      G1Proj t;
      for (int l = 0; l < BN_NL; l++) { t.x.v[l] = rows[27 * cc + l]; t.y.v[l] = rows[27 * cc + 9 + l]; t.z.v[l] = rows[27 * cc + 18 + l]; }
      BN_SETB(t.x, 3.0, 0.5); BN_SETB(t.y, 3.0, 0.5); BN_SETB(t.z, 3.0, 0.5);
      L[q] = g1_add(L[q], t);
    }
  }
  for (int m = 1; m < lpi; m <<= 1) {
    G1Proj N[4];
    for (int q = 0; q < lpi; q++) N[q] = g1_add(L[q], L[q ^ m]);
    for (int q = 0; q < lpi; q++) L[q] = N[q];
  }
  g1_out(out, L[0]);
  return 1;
}
