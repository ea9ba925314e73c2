// bn254_pairing_rlc.h -- BN254_FLAG_RLC for the batch pairing product (include/bn254_verify.h, bn254_pairing_check_batch_flags): what the kernels of
// bn254_k_pairing_rlc.hip, the host code of bn254_capi_pairing_rlc.hip and the host compile behind bn254_dbg_pairing_batch_rlc(device = -1) share.
// One launch of m items of n_pairs positions, V the variable and S the shared ones:
//   load      the loader of the exact entry; phase 1 is decided before any weight exists
//   weights   every pending item i draws an odd 128-bit weight r_i and every finite G1 point of it becomes r_i P_ij in the workspace (pb_rlc_weigh_item)
//   items     the Miller loop over V alone, no final exponentiation: f_i stays in VE_F; the r-torsion tests of the variable G2 points decide as in the exact entry
//   groups    per 64 consecutive items: for every position of S the sum of the pending items' weighted points, and the product F_g of their f_i, into a GROUP
//             workspace whose item has the positions of S alone, compacted (position t of the group item is the t-th shared position, so the prepared records
//             serve it as they stand and every one of its positions is shared)
//   check     per group: the table-driven Miller loop over its |S| positions, times F_g, the final exponentiation, the compare with 1
//   scatter   a pending item of a group that passed is accepted; the items of a failed group go through the exact check on their WEIGHTED points: r_i is invertible
//             mod r and GT has prime order r, so prod_j e(r_i P_ij, Q_ij) = (prod_j e(P_ij, Q_ij))^(r_i) is 1 exactly when the unweighted product is.
#pragma once
#include "bn254_pairing_batch.h"
#include "bn254_rlc.h"

namespace bn254 {

#define PB_RLC_GROUP 64
// the elements of a GROUP item that hold F_g until the check multiplies it in: T of pair 0, which a table-driven run never touches
#define PB_RLC_FG_ELEM VE_S0

// the weight of item i of a launch: the first 128 bits of block i of the call's ChaCha20 stream, forced odd (bn254_kzg.h::kzg_weight)
BN_HD void pb_rlc_weight(uint32_t out[4], const ChaChaKey& key, uint32_t i) {
  chacha20_block4(out, key, i);
  out[0] |= 1u;
}
// r P for a finite affine P and a 128-bit r != 0: double and always add (complete formulas, the addition selected by the bit), then to affine
BN_HD G1Aff pb_rlc_mul(const G1Aff& P, const uint32_t wgt[4]) {
  G1Proj acc = g1_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int wi = 3; wi >= 0; wi--) {
    const uint32_t word = wi == 3 ? wgt[3] : wi == 2 ? wgt[2] : wi == 1 ? wgt[1] : wgt[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 31; bit >= 0; bit--) {
      acc = g1_dbl(acc);
      const G1Proj t = g1_add_mixed(acc, P);
      const bool on = ((word >> bit) & 1u) != 0;
      acc.x = fp_reduce(fp_select(on, t.x, acc.x)); acc.y = fp_reduce(fp_select(on, t.y, acc.y)); acc.z = fp_reduce(fp_select(on, t.z, acc.z));
    }
  }
  return g1_to_affine(acc);
}
// every finite G1 point of a loaded item times the item's weight, in place.  G1 has cofactor 1 and r_i is odd and below r, so no identity bit changes
template <class W>
BN_HD void pb_rlc_weigh_item(W& w, int np, const uint32_t wgt[4], bool live) {
  const uint32_t ident = pb_ident(w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int j = 0; j < np; j++) {
    G1Aff P; P.x = w.ld(vp_p(j)); P.y = w.ld(vp_p(j) + 1);
    const G1Aff Q = pb_rlc_mul(P, wgt);
    if (live && !((ident >> (2 * j)) & 1u)) { w.st(vp_p(j), Q.x); w.st(vp_p(j) + 1, Q.y); }
  }
}
// vm_miller_run_var over a SUBSET of the positions (bit j of var_mask: position j takes part; wave-uniform): the Miller loop of the variable positions of an item with
// shared ones, which contribute nothing here.  The loops keep vm_miller_run_var's shape -- a count and a uniform test per position -- and its two code regions
template <class W, class KINDS>
BN_HD int vm_miller_run_sub(W& w, const KINDS& kinds, int s_begin, int s_end, int np, uint32_t var_mask, uint32_t ident, int e, int fold = 0) {
  Fp2 f4, f5;
  if ((fold & MR_FOLD_INIT) && s_begin == 0) {
    w.park(0, fp2_one()); w.park(1, fp2_zero()); w.park(2, fp2_zero()); w.park(3, fp2_zero());
    f4 = fp2_zero(); f5 = fp2_zero();
    for (int j = 0; j < np; j++) { const int et = vp_t(j), eb = vp_q(j); vst2(w, et, vld2(w, eb)); vst2(w, et + 2, vld2(w, eb + 2)); vst2(w, et + 4, fp2_one()); }
  } else mf_load(w, e, f4, f5);
  for (int s = s_begin; s < s_end; s++) {
    const int kind = kinds.get(s);
    if (kind == 0) {
      if (s != 0) mf_sqr(w, f4, f5);
      for (int j = 0; j < np; j++) {
        if (!((var_mask >> j) & 1u)) continue;
        BN_SCHED_FENCE();
        G2Line l = mf_g2(w, 0, vp_t(j), vp_q(j));
        mf_line_var_sel(w, l, vp_p(j), vp_skips(ident, j), f4, f5);
      }
    } else {
      for (int j = 0; j < np; j++) {
        if (!((var_mask >> j) & 1u)) continue;
        BN_SCHED_FENCE();
        G2Line l = mf_g2(w, kind, vp_t(j), vp_q(j));
        mf_line_var_sel(w, l, vp_p(j), vp_skips(ident, j), f4, f5);
      }
    }
    BN_SCHED_FENCE();
  }
  mf_store(w, e, f4, f5);
  int failed = -1;
  if ((fold & MR_FOLD_ATE) && s_end == BN_ATE_STEPS)
    for (int j = 0; j < np; j++) {
      if (!((var_mask >> j) & 1u)) continue;
      const bool ok = vm_g2_ate_check(w, vp_t(j), vp_q(j));
      if (failed < 0 && vp_q_finite(ident, j) && !ok) failed = j;
    }
  return failed;
}
// the Fp12 at element e of a workspace item (k-order storage) as a tower value, and back
template <class W> BN_HD Fp12 pb_rlc_ld12(W& w, int e) { Fp12 f; f.c0 = vld_half(w, e, 0); f.c1 = vld_half(w, e, 1); return fp12_reduce(f); }
template <class W> BN_HD void pb_rlc_st12(W& w, int e, const Fp12& f) { vst_half(w, e, 0, f.c0); vst_half(w, e, 1, f.c1); }
BN_HD Fp12 pb_rlc_mul12(const Fp12& a, const Fp12& b) { return fp12_reduce(fp12_mul(a, b)); }
// what lane 0 of a group's wavefront leaves in the group item beside the sums: the G2 points of the shared positions as pb_load_item_shared stores them (the
// cooperative form of the check reads them), compacted, and the identity bits.  p_inf: bit t set when the sum of shared position t is the identity
template <class W>
BN_HD void pb_rlc_group_finish(W& gw, uint32_t mask, const int32_t* prepared, uint32_t p_inf) {
  uint32_t ident = 0;
  int t = 0;
  for (uint32_t m = mask; m; m &= m - 1, t++) {
    const int32_t* h = prepared + (size_t)t * PB_PREP_DWORDS;
    if ((uint32_t)h[2] & PB_PREP_FLAG_IDENTITY) ident |= 2u << (2 * t);
    if ((p_inf >> t) & 1u) ident |= 1u << (2 * t);
    for (int c = 0; c < 4; c++) gw.st(vp_q(t) + c, pb_rec_fp(h + PB_PREP_HDR_DWORDS + c * BN_NL));
  }
  Fp v = fp_zero();
  v.v[0] = (int32_t)ident;
  gw.st(VP_IDENT, v);
}

// ---- launches (bn254_k_pairing_rlc.hip): everything between the loader and the scatter -----------------------------------------------------------------------------
struct PairingRlcArgs {
  int n_pairs; unsigned shared_mask; const int32_t* prepared;   // as PairingLaunchArgs; the records' headers were checked by the loader (a bad one leaves no item pending)
  size_t n;                                   // items of this launch
  int32_t* ws; uint8_t* status;               // what the loader left
  int32_t* grp_ws; uint8_t* grp_status;       // ceil(n / 64) items and bytes
  const uint32_t* weights; ChaChaKey wkey;    // the probe's weights (n x 4 words), or null: the ChaCha20 stream of wkey
  const int32_t* one;                         // 1 in GT
  int grp_form;                               // the form of the group check (bn254_g16_plan.h: PAIRING_FORM_LANES or _COOP)
  uint8_t* out_grp_gt = nullptr;              // the probe: ceil(n / 64) x 384 bytes
};

}  // namespace bn254

hipError_t bn254_launch_pairing_rlc_joint(const bn254::PairingRlcArgs& a, hipStream_t s);
