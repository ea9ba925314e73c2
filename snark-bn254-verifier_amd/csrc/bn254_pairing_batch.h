// bn254_pairing_batch.h -- the batch pairing product over caller-supplied pairs (include/bn254_verify.h, bn254_pairing_check_batch): what the kernels of
// bn254_k_pairing.hip and the host compile behind bn254_dbg_pairing_batch(device = -1) share.  Host- and device-compilable, templated on the workspace accessor
// like bn254_vm.h: the loader of one item (range and on-curve checks in record order, the points and the identity bits into the workspace), and the whole item on a
// plain-array accessor -- loader, vm_miller_run_var, vm_final_exp_program, the compare with 1 -- so that the operation sequence the GPU runs is checked against the
// oracle without one.
// Two forms of the launches: the LANE form (one item per lane, bn254_k_pairing.hip) and, for small batches, which leave most of the GPU idle in the lane form, the
// cooperative twelve-lane form (bn254_coop12.hip::k_coop12_miller_pairs after the same loader).  bn254_g16_plan.h::pairing_form chooses; the status and GT bytes are
// the same.
// Items with shared, prepared G2 points (bn254_pairing_check_batch_shared): the layout of a prepared record, the loader of the packed item (pb_load_item_shared) and
// the whole item on plain arrays with the mixed run (pb_item_shared_on_host, bn254_vm.h::vm_miller_run_mix).
#pragma once
#include "bn254_vm.h"
#include "bn254_kernels.h"

namespace bn254 {

#define PB_PAIR_LEN 192          // G1 x | y, then G2 x.c1 | x.c0 | y.c1 | y.c0, 32-byte big-endian each (BN254_PAIRING_PAIR_LEN)
#define PB_MAX_PAIRS VP_MAX_PAIRS

// 32 big-endian bytes -> little-endian words; aligned: p is 4-byte aligned (dword loads)
BN_HD void pb_field_words(uint32_t w[8], const uint8_t* p, bool aligned) {
  if (aligned) {
    const uint32_t* d = (const uint32_t*)p;
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = __builtin_bswap32(d[7 - i]);
  } else words_from_be(w, p);
}
BN_HD bool pb_words_zero(const uint32_t w[8]) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= w[i];
  return o == 0;
}
// One field of a record: the Montgomery form of its value (mod p), whether it is canonical, whether it is zero
BN_HD Fp pb_field(const uint8_t* p, bool aligned, bool& memb, bool& zero) {
  uint32_t w[8];
  pb_field_words(w, p, aligned);
  memb &= !words_ge(w, BN_P_WORDS);
  zero &= pb_words_zero(w);
  return fp_from_words(w);
}
// Phase 1 of the definition: the np records of one item in record order (pair 0 G1, pair 0 G2, pair 1 G1, ...).  The first failure decides: a coordinate >= p is
// NOT_MEMBER, otherwise a point off its curve NOT_ON_CURVE; an all-zero point is the identity (its bit goes to VP_IDENT) and is on no curve equation.  Every point is
// stored whatever the outcome (a decided item is never read again).  Returns the decided error, or BN254_ST_PENDING.
template <class W>
BN_HD int pb_load_item(W& w, const uint8_t* rec, int np, bool aligned) {
  int err = 0;
  uint32_t ident = 0;
  for (int j = 0; j < np; j++) {
    const uint8_t* r = rec + (size_t)PB_PAIR_LEN * j;
    {
      bool memb = true, zero = true;
      G1Aff P;
      P.x = pb_field(r, aligned, memb, zero); P.y = pb_field(r + 32, aligned, memb, zero);
      if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!zero && !g1_on_curve(P)) err = BN254_ST_NOT_ON_CURVE; }
      if (zero) ident |= 1u << (2 * j);
      w.st(vp_p(j), P.x); w.st(vp_p(j) + 1, P.y);
    }
    {
      bool memb = true, zero = true;
      G2Aff Q;
      Q.x.c1 = pb_field(r + 64, aligned, memb, zero); Q.x.c0 = pb_field(r + 96, aligned, memb, zero);
      Q.y.c1 = pb_field(r + 128, aligned, memb, zero); Q.y.c0 = pb_field(r + 160, aligned, memb, zero);
      if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!zero && !g2_on_curve(Q)) err = BN254_ST_NOT_ON_CURVE; }
      if (zero) ident |= 2u << (2 * j);
      vst2(w, vp_q(j), Q.x); vst2(w, vp_q(j) + 2, Q.y);
    }
  }
  Fp m = fp_zero();
  m.v[0] = (int32_t)ident;
  w.st(VP_IDENT, m);
  return err ? err : BN254_ST_PENDING;
}
template <class W> BN_HD uint32_t pb_ident(W& w) { return (uint32_t)w.ld(VP_IDENT).v[0]; }

// ---- shared, prepared G2 points (bn254_g2_prepare, bn254_pairing_check_batch_shared) -------------------------------------------------------------------------------
// A prepared record is plain data the caller owns: PB_PREP_HDR_DWORDS header words (magic, layout version, flags -- bit 0: the point is the identity -- and a reserved
// word), the affine point as the four Fp the loader would have stored for its 128 bytes (x.c0 x.c1 y.c0 y.c1, the workspace layout), and the BN_ATE_STEPS line
// entries of FIXED_LINE_DWORDS dwords in the encoding of the key tables (m | c | xi c).  A record is valid for the layout version that wrote it and no other.
#define PB_PREP_MAGIC 0x50324742u      // "BG2P"
#define PB_PREP_VERSION 1u
#define PB_PREP_FLAG_IDENTITY 1u
#define PB_PREP_HDR_DWORDS 4
#define PB_PREP_POINT_DWORDS (4 * BN_NL)
#define PB_PREP_DWORDS (PB_PREP_HDR_DWORDS + PB_PREP_POINT_DWORDS + BN_ATE_STEPS * FIXED_LINE_DWORDS)
#define PB_PREP_LEN ((size_t)PB_PREP_DWORDS * 4)
static_assert(sizeof(((Fp*)0)->v) == BN_NL * 4 && FIXED_LINE_DWORDS == 6 * BN_NL, "a record holds the digits of four Fp and of three Fp2 per line");
#define PB_G1_LEN 64             // a shared position of a packed item: G1 x | y alone

// bytes of a packed item: a shared position (bit j of mask) is PB_G1_LEN bytes, a variable one PB_PAIR_LEN
BN_HD size_t pb_item_len(int np, uint32_t mask) { return (size_t)PB_PAIR_LEN * (size_t)np - (size_t)(PB_PAIR_LEN - PB_G1_LEN) * (size_t)__builtin_popcount(mask & ((1u << np) - 1u)); }
// one Fp of a record: its digits as stored (wave-uniform address on the GPU: scalar loads)
BN_HD Fp pb_rec_fp(const int32_t* p) {
  Fp r;
#pragma unroll
  for (int l = 0; l < BN_NL; l++) r.v[l] = p[l];
  BN_SETB(r, 1.2, 0.5);
  return r;
}
BN_HD Fp2 pb_rec_fp2(const int32_t* p) { Fp2 r; r.c0 = pb_rec_fp(p); r.c1 = pb_rec_fp(p + BN_NL); return r; }
BN_HD bool pb_records_ok(const int32_t* prepared, uint32_t mask) {
  bool ok = true;
  int t = 0;
  for (uint32_t m = mask; m; m &= m - 1, t++) {
    const int32_t* h = prepared + (size_t)t * PB_PREP_DWORDS;
    ok &= (uint32_t)h[0] == PB_PREP_MAGIC && (uint32_t)h[1] == PB_PREP_VERSION;
  }
  return ok;
}
// pb_load_item on the PACKED record of an item with shared positions (mask, np > bit): phase 1 in record order over what the record holds -- for a shared position
// the G1 point alone -- and for a shared position the affine point and the identity flag of its prepared record (prepared: the records of the shared positions in
// ascending order, headers checked by the caller) into vp_q(j) and VP_IDENT.  Afterwards the workspace is what pb_load_item leaves for the expanded item, in which
// every shared position carries the 128 bytes its record was prepared from.
template <class W>
BN_HD int pb_load_item_shared(W& w, const uint8_t* rec, int np, uint32_t mask, const int32_t* prepared, bool aligned) {
  int err = 0;
  uint32_t ident = 0;
  const uint8_t* r = rec;
  int t = 0;
  for (int j = 0; j < np; j++) {
    {
      bool memb = true, zero = true;
      G1Aff P;
      P.x = pb_field(r, aligned, memb, zero); P.y = pb_field(r + 32, aligned, memb, zero);
      if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!zero && !g1_on_curve(P)) err = BN254_ST_NOT_ON_CURVE; }
      if (zero) ident |= 1u << (2 * j);
      w.st(vp_p(j), P.x); w.st(vp_p(j) + 1, P.y);
    }
    if ((mask >> j) & 1u) {
      const int32_t* h = prepared + (size_t)t * PB_PREP_DWORDS;
      if ((uint32_t)h[2] & PB_PREP_FLAG_IDENTITY) ident |= 2u << (2 * j);
      for (int c = 0; c < 4; c++) w.st(vp_q(j) + c, pb_rec_fp(h + PB_PREP_HDR_DWORDS + c * BN_NL));
      t++;
      r += PB_G1_LEN;
    } else {
      bool memb = true, zero = true;
      G2Aff Q;
      Q.x.c1 = pb_field(r + 64, aligned, memb, zero); Q.x.c0 = pb_field(r + 96, aligned, memb, zero);
      Q.y.c1 = pb_field(r + 128, aligned, memb, zero); Q.y.c0 = pb_field(r + 160, aligned, memb, zero);
      if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!zero && !g2_on_curve(Q)) err = BN254_ST_NOT_ON_CURVE; }
      if (zero) ident |= 2u << (2 * j);
      vst2(w, vp_q(j), Q.x); vst2(w, vp_q(j) + 2, Q.y);
      r += PB_PAIR_LEN;
    }
  }
  Fp m = fp_zero();
  m.v[0] = (int32_t)ident;
  w.st(VP_IDENT, m);
  return err ? err : BN254_ST_PENDING;
}
// the line tables of the shared positions: table t is that of the t-th shared position (plain loads here; the kernels read the same dwords by scalar loads)
struct PbRecLines {
  const int32_t* prepared;
  BN_HD FixedLine get(int t, int s) const {
    const int32_t* e = prepared + (size_t)t * PB_PREP_DWORDS + PB_PREP_HDR_DWORDS + PB_PREP_POINT_DWORDS + (size_t)s * FIXED_LINE_DWORDS;
    FixedLine l; l.m = pb_rec_fp2(e); l.c = pb_rec_fp2(e + 2 * BN_NL); l.xc = pb_rec_fp2(e + 4 * BN_NL);
    return l;
  }
};

// ---- the host compile: one item on plain arrays ------------------------------------------------------------------------------------------------------------
struct PbHostLane {
  Fp e[VE_COUNT];
  Fp2 slot[4];
  Fp ld(int i) const { return e[i]; }
  void st(int i, const Fp& a) { e[i] = a; }
  void park(int s, const Fp2& a) { slot[s] = a; }
  Fp2 unpark(int s) const { return slot[s]; }
};
struct PbHostKinds { uint8_t kind[BN_ATE_STEPS]; PbHostKinds() { for (int s = 0; s < BN_ATE_STEPS; s++) kind[s] = (uint8_t)miller_step_kind(s); } int get(int s) const { return kind[s]; } };
struct PbHostOps {   // the operations vm_final_exp_program asks for
  PbHostLane& w;
  void f12_mul(int d, int a, int b, bool conj_b = false) { vm_f12_mul(w, d, a, b, conj_b); }
  void f12_cyclo_sqr(int d, int a) { vm_f12_cyclo_sqr(w, d, a); }
  void f12_cyclo_sqr_n(int d, int a, int count) { vm_f12_cyclo_sqr_n(w, d, a, count); }
  void f12_frob(int d, int a, int j) { vm_f12_frob(w, d, a, j); }
  void f12_inv(int d, int a) { vm_f12_inv(w, d, a); }
};
// The item's status as bn254_pairing_check_batch defines it; out_gt (may be null): the final-exponentiated product in the 384-byte format 0 of bn254_dbg_pairing,
// written when the item reached the pairing.  run_steps: Miller steps per run, as the launcher cuts the loop (BN_ATE_STEPS: one run).
inline uint8_t pb_item_on_host(const uint8_t* rec, int np, uint8_t* out_gt, int run_steps = BN_ATE_STEPS) {
  static const PbHostKinds kinds;
  PbHostLane w;
  for (auto& x : w.e) x = fp_zero();
  int st = pb_load_item(w, rec, np, false);
  if (!(st & BN254_ST_PENDING)) return (uint8_t)st;
  const uint32_t ident = pb_ident(w);
  if (run_steps < 1) run_steps = 1;
  int failed = -1;
  for (int s = 0; s < BN_ATE_STEPS; s += run_steps) {
    const int r = vm_miller_run_var(w, kinds, s, s + run_steps < BN_ATE_STEPS ? s + run_steps : BN_ATE_STEPS, np, ident, VE_F, MR_FOLD_INIT | MR_FOLD_ATE);
    if (failed < 0) failed = r;
  }
  if (failed >= 0) return BN254_ST_NOT_IN_SUBGROUP;
  PbHostOps ops{w};
  vm_final_exp_program(ops);
  if (out_gt) {
    const int korder[6] = {0, 2, 4, 1, 3, 5};
    for (int t = 0; t < 6; t++)
      for (int h = 0; h < 2; h++) { uint32_t v[8]; fp_to_words(v, w.ld(VE_S0 + 2 * korder[t] + h)); words_to_be(out_gt + 64 * t + 32 * h, v); }
  }
  int32_t one[12 * BN_NL] = {0};
  for (int l = 0; l < BN_NL; l++) one[l] = BN_ONE[l];
  return vm_f12_eq_const(w, VE_S0, one) ? BN254_ST_ACCEPT : BN254_ST_REJECT;
}

// pb_item_on_host for the packed record of an item with shared positions: pb_load_item_shared, vm_miller_run_mix, the same final exponentiation and compare.
// prepared: the records of the shared positions, headers checked by the caller
// the part of pb_item_shared_on_host behind the loader: a lane whose points and identity bits are in place (bn254_kzg.h fills one from the G1 walk)
inline uint8_t pb_lane_shared_on_host(PbHostLane& w, int np, uint32_t mask, const int32_t* prepared, uint8_t* out_gt, int run_steps = BN_ATE_STEPS) {
  static const PbHostKinds kinds;
  const uint32_t all = (1u << np) - 1u;
  const uint32_t ident = pb_ident(w);
  if (run_steps < 1) run_steps = 1;
  const PbRecLines lines{prepared};
  int failed = -1;
  for (int s = 0; s < BN_ATE_STEPS; s += run_steps) {
    const int s1 = s + run_steps < BN_ATE_STEPS ? s + run_steps : BN_ATE_STEPS;
    const int r = (all & ~mask) ? vm_miller_run_mix<true>(w, lines, kinds, s, s1, all & ~mask, all & mask, ident, VE_F, MR_FOLD_INIT | MR_FOLD_ATE)
                                : vm_miller_run_mix<false>(w, lines, kinds, s, s1, 0u, all & mask, ident, VE_F, MR_FOLD_INIT | MR_FOLD_ATE);
    if (failed < 0) failed = r;
  }
  if (failed >= 0) return BN254_ST_NOT_IN_SUBGROUP;
  PbHostOps ops{w};
  vm_final_exp_program(ops);
  if (out_gt) {
    const int korder[6] = {0, 2, 4, 1, 3, 5};
    for (int t = 0; t < 6; t++)
      for (int h = 0; h < 2; h++) { uint32_t v[8]; fp_to_words(v, w.ld(VE_S0 + 2 * korder[t] + h)); words_to_be(out_gt + 64 * t + 32 * h, v); }
  }
  int32_t one[12 * BN_NL] = {0};
  for (int l = 0; l < BN_NL; l++) one[l] = BN_ONE[l];
  return vm_f12_eq_const(w, VE_S0, one) ? BN254_ST_ACCEPT : BN254_ST_REJECT;
}
inline uint8_t pb_item_shared_on_host(const uint8_t* rec, int np, uint32_t mask, const int32_t* prepared, uint8_t* out_gt, int run_steps = BN_ATE_STEPS) {
  PbHostLane w;
  for (auto& x : w.e) x = fp_zero();
  const uint32_t all = (1u << np) - 1u;
  int st = pb_load_item_shared(w, rec, np, mask & all, prepared, false);
  if (!(st & BN254_ST_PENDING)) return (uint8_t)st;
  return pb_lane_shared_on_host(w, np, mask, prepared, out_gt, run_steps);
}

// ---- the launches of one pass (bn254_k_pairing.hip): load, the Miller loop in runs, the final exponentiation, the tail ----------------------------------------
struct PairingLaunchArgs {
  const uint8_t* pairs; size_t item_stride;   // device memory: item i at pairs + i * item_stride, n_pairs records of PB_PAIR_LEN bytes (shared_mask: packed)
  int n_pairs;                                // 1 .. PB_MAX_PAIRS
  size_t n;                                   // items of this launch, <= G16_MAX_LAUNCH
  int32_t* ws;                                // G16_WS_BYTES_PER_PROOF * n bytes
  uint8_t* status;                            // n bytes
  const int32_t* one;                         // 108 dwords: 1 in GT (the verdict tail's target); null: no verdict
  uint8_t* out_gt;                            // n x 384 bytes (the store tail), or null.  With a store tail AND a verdict the status bytes are the verdict's; with the
                                              // store tail alone a pending item ends as BN254_ST_ACCEPT ("the value is valid")
  int form = 0;                               // bn254_g16_plan.h: PAIRING_FORM_PLAN (pairing_form at the default threshold), _LANES, _COOP (n <= COOP12_MAX_PROOFS)
  unsigned shared_mask = 0;                   // bit j: position j's G2 is shared; then the items are PACKED (pb_item_len) and
  const int32_t* prepared = nullptr;          // device memory, 4-byte aligned: popcount(shared_mask) records of PB_PREP_LEN bytes, ascending position order
  bool skip_load = false;                     // the workspace and the status bytes are what a loader left already (bn254_kzg.h: the G1 points come from the G1 walk);
                                              // pairs / item_stride are not read.  Every launch behind the load step is the same
  // A launch cut into its parts (bn254_pairing_rlc.h; none of them set: the whole launch).  load_only: the loader alone.  miller_only (lane form): the loader unless
  // skipped, then the Miller runs with the r-torsion tests; f stays in VE_F.  skip_miller: the final exponentiation of VE_F in the launch's form and the tails.
  bool load_only = false, miller_only = false, skip_miller = false;
};

}  // namespace bn254

hipError_t bn254_launch_pairing_batch(const bn254::PairingLaunchArgs& a, hipStream_t s);
