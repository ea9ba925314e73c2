// tests/hostsim/hostsim_fused.cpp -- TEST HARNESS: hostsim.cpp (the product's device arithmetic compiled for the host with the bound
// tracker on) plus the entry points tests/test_gpu_fused_tail.py needs for the operations that ride on their neighbours:
//   - the final exponentiation program without conjugation operations (VE_CONJ on the consumer's load), beside the sequence with
//     explicit conjugations it replaced, down to the digits of VE_S0;
//   - a whole Groth16 pairing check with f = 1 / T = (B, 1), the r-torsion test of B and the comparison with the target either as
//     operations of their own or folded into the run that starts the loop, the run that ends it and the last product.
// Built by the test into libhostsim_fused.so; not part of the product.
#define HS_WITH_CURVE 1
#include "hostsim.cpp"

namespace {
const int KORDER[6] = {0, 2, 4, 1, 3, 5};   // tower byte order c0 = (k0, k2, k4), c1 = (k1, k3, k5) -> k index
void f12_to_ws(HostWs& w, int e, const uint8_t* b, int inflate) {
  for (int t = 0; t < 6; t++) { w.el[e + 2 * KORDER[t]] = fp_in(b + 64 * t, inflate); w.el[e + 2 * KORDER[t] + 1] = fp_in(b + 64 * t + 32, -inflate); }
}
void ws_to_f12(uint8_t* o, HostWs& w, int e) {
  for (int t = 0; t < 6; t++) { fp_out(o + 64 * t, w.el[e + 2 * KORDER[t]]); fp_out(o + 64 * t + 32, w.el[e + 2 * KORDER[t] + 1]); }
}
// the final exponentiation with every conjugation an operation of its own: the sequence vm_final_exp_program had before
template <class OPS>
void final_exp_explicit_conj(OPS& ops) {
  ops.f12_inv(VE_S0, VE_F);
  ops.f12_conj(VE_S1, VE_F);
  ops.f12_mul(VE_S0, VE_S1, VE_S0, false);
  ops.f12_frob(VE_S1, VE_S0, 2);
  ops.f12_mul(VE_F, VE_S1, VE_S0);
  vm_exp_u(ops, VE_S0, VE_F); ops.f12_conj(VE_S0, VE_S0);
  ops.f12_cyclo_sqr(VE_S0, VE_S0);
  ops.f12_cyclo_sqr(VE_S1, VE_S0);
  ops.f12_mul(VE_S1, VE_S0, VE_S1);
  vm_exp_u(ops, VE_S2, VE_S1); ops.f12_conj(VE_S2, VE_S2);
  ops.f12_conj(VE_S3, VE_S1);
  ops.f12_mul(VE_S1, VE_S2, VE_S3);
  ops.f12_cyclo_sqr(VE_S3, VE_S2);
  vm_exp_u(ops, VE_S4, VE_S3);
  ops.f12_mul(VE_S4, VE_S1, VE_S4);
  ops.f12_mul(VE_S3, VE_S0, VE_S4);
  ops.f12_mul(VE_S0, VE_S2, VE_S4);
  ops.f12_mul(VE_S0, VE_F, VE_S0);
  ops.f12_frob(VE_S2, VE_S3, 1); ops.f12_mul(VE_S0, VE_S2, VE_S0);
  ops.f12_frob(VE_S2, VE_S4, 2); ops.f12_mul(VE_S0, VE_S2, VE_S0);
  ops.f12_conj(VE_S2, VE_F); ops.f12_mul(VE_S2, VE_S2, VE_S3);
  ops.f12_frob(VE_S2, VE_S2, 3);
  ops.f12_mul(VE_S0, VE_S2, VE_S0);
}
}  // namespace

extern "C" {
// which: 0 vm_final_exp_program, 1 the sequence with explicit conjugations.  o: the result, canonical bytes in tower order; digits: the 12 x BN_NL
// digits of VE_S0 as the program left them (k-order), unreduced
void hs_vm_final_exp(int which, uint8_t* o, int32_t* digits, const uint8_t* f, int inflate) {
  static HostWs w;
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
  f12_to_ws(w, VE_F, f, inflate);
  HostOps ops{w, {nullptr, nullptr}, false};
  if (which == 0) vm_final_exp_program(ops); else final_exp_explicit_conj(ops);
  ws_to_f12(o, w, VE_S0);
  for (int k = 0; k < 12; k++) for (int l = 0; l < BN_NL; l++) digits[k * BN_NL + l] = w.el[VE_S0 + k].v[l];
}

// One Groth16 pairing check e(pa, qb) e(pl, qg) e(pc, qd) == target on the VM, the Miller loop in runs of per_run steps (0: the whole loop).
// folded 0: f = 1 and T = (B, 1) stored beforehand, vm_g2_ate_check after the loop, vm_final_exp_program, vm_f12_eq_const -- the separate operations.
// folded 1: VE_F and VE_T hold junk; the runs carry MR_FOLD_INIT | MR_FOLD_ATE, the program stops before its last product and vm_f12_mul_eq_const ends it.
// Returns bit 0: B passed the r-torsion test, bit 1: the product equals the target; -1: a line table could not be built.  o: VE_S0, canonical, tower order.
int hs_vm_g16_verdict(int folded, int per_run, const uint8_t* pa, const uint8_t* qb, const uint8_t* pl, const uint8_t* qg, const uint8_t* pc, const uint8_t* qd, int l_inf,
                      const uint8_t* target, uint8_t* o) {
  static FixedLine tg[BN_ATE_STEPS], td[BN_ATE_STEPS];
  if (!fixed_line_table(tg, g2_in(qg)) || !fixed_line_table(td, g2_in(qd))) return -1;
  static HostWs w;
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
  put_g1(w, VE_AX, g1_in(pa)); put_g1(w, VE_CX, g1_in(pc));
  G1Aff L = g1_in(pl);
  if (l_inf) { L.x = fp_zero(); L.y = fp_one(); }
  put_g1(w, VE_LX, L);
  G2Aff B = g2_in(qb);
  w.el[VE_B] = B.x.c0; w.el[VE_B + 1] = B.x.c1; w.el[VE_B + 2] = B.y.c0; w.el[VE_B + 3] = B.y.c1;
  int32_t tgt[12 * BN_NL];
  {
    static HostWs t;
    f12_to_ws(t, 0, target, 0);
    for (int k = 0; k < 12; k++) for (int l = 0; l < BN_NL; l++) tgt[k * BN_NL + l] = t.el[k].v[l];
  }
  HostOps ops{w, {tg, td}, l_inf != 0};
  if (per_run <= 0) per_run = BN_ATE_STEPS;
  bool in_g2 = true, accept;
  if (!folded) {
    w.el[VE_F] = fp_one();
    w.el[VE_T] = B.x.c0; w.el[VE_T + 1] = B.x.c1; w.el[VE_T + 2] = B.y.c0; w.el[VE_T + 3] = B.y.c1; w.el[VE_T + 4] = fp_one();
    vm_miller_program_runs(ops, per_run);
    in_g2 = vm_g2_ate_check(w, VE_T, VE_B);
    vm_final_exp_program(ops);
    accept = vm_f12_eq_const(w, VE_S0, tgt);
  } else {
    const Fp junk = g1_in(pa).x;
    for (int e = 0; e < 12; e++) w.el[VE_F + e] = junk;
    for (int e = 0; e < 6; e++) w.el[VE_T + e] = junk;
    const FixedLine* tabs[2] = {tg, td};
    HostOps::Lines lines{tabs};
    for (int s = 0; s < BN_ATE_STEPS; s += per_run)
      in_g2 &= vm_miller_run(w, lines, HostOps::Kinds{}, s, s + per_run < BN_ATE_STEPS ? s + per_run : BN_ATE_STEPS, VE_T, VE_B, VE_F, VE_AX, VE_LX, l_inf != 0, VE_CX, false,
                             MR_FOLD_INIT | MR_FOLD_ATE);
    vm_final_exp_program_head(ops);
    accept = vm_f12_mul_eq_const(w, VE_S0, VE_S2, VE_S0, tgt);
  }
  ws_to_f12(o, w, VE_S0);
  return (in_g2 ? 1 : 0) | (accept ? 2 : 0);
}
}
