// bn254_k_pairing_rlc.hip -- BN254_FLAG_RLC for the batch pairing product (include/bn254_verify.h, bn254_pairing_check_batch_flags; bn254_pairing_rlc.h): the kernels
// between the loader of the exact entry and the scatter, and the launches of the joint check.
//   k_pairing_rlc_weigh       one item per lane: the item's odd 128-bit weight (ChaCha20 block i, or the probe's), every finite G1 point times it, in place
//   k_miller_run_sub          k_miller_run_var over a SUBSET of the positions (a wave-uniform mask argument): the variable ones alone, no table read, f left in VE_F, the
//                             r-torsion tests of the variable G2 points at the loop's end (bn254_pairing_rlc.h::vm_miller_run_sub).  The doubling and the addition side
//                             keep their own G2 formulas and line product: no code region is joined
//   k_pairing_rlc_group_sums  one wavefront per group of 64 items: for the t-th shared position the sum of the pending items' weighted points (six butterfly rounds of
//                             complete additions), affine, to position t of the GROUP item; lane 0 also writes the group's G2 points, identity bits and status byte
//   k_pairing_rlc_group_prod  one wavefront per group: the product of the pending items' f_i (six butterfly rounds of Fp12 products, 1 for a lane that is not pending)
// The group check itself is the launches of bn254_k_pairing.hip on the group workspace: the all-shared table-driven run, k_f12_mul by F_g, the final exponentiation in
// the launch's form and k_g16_compare.
#include <hip/hip_runtime.h>
#include "bn254_launch_ops.h"
#include "bn254_g16_plan.h"
#include "bn254_pairing_rlc.h"

namespace bn254 {

__global__ void __launch_bounds__(256, 2) k_pairing_rlc_weigh(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int n_pairs, const uint32_t* __restrict__ weights,
                                                              ChaChaKey wkey) {
  VM_KERNEL_PROLOGUE();
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > PB_MAX_PAIRS ? PB_MAX_PAIRS : np);
  uint32_t wgt[4];
  if (weights) {
    const uint32_t ii = i < n ? i : n - 1;
#pragma unroll
    for (int q = 0; q < 4; q++) wgt[q] = weights[(size_t)ii * 4 + q];
    wgt[0] |= 1u;
  } else pb_rlc_weight(wgt, wkey, i);
  pb_rlc_weigh_item(w, np, wgt, i < n && (st & BN254_ST_PENDING) != 0);
}

struct SubKinds {   // the step table, two steps per byte, by value in the kernel arguments (bn254_k_pairing.hip::PairKinds)
  MillerKinds k;
  __device__ __forceinline__ int get(int s) const { return __builtin_amdgcn_readfirstlane((k.nib[s >> 1] >> ((s & 1) * 4)) & 15); }
};
__global__ void __launch_bounds__(256, 2) k_miller_run_sub(int32_t* ws, uint32_t n, uint8_t* status, MillerKinds kinds, int s_begin, int s_end, int n_pairs, uint32_t var_mask, int e, int fold) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  SubKinds pk{kinds};
  const int s_last = __builtin_amdgcn_readfirstlane(s_end), fl = __builtin_amdgcn_readfirstlane(fold);
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > PB_MAX_PAIRS ? PB_MAX_PAIRS : np);
  const uint32_t vm = (uint32_t)__builtin_amdgcn_readfirstlane((int)var_mask) & ((1u << np) - 1u);
  const uint32_t ident = pb_ident(w);
  const int failed = vm_miller_run_sub(w, pk, __builtin_amdgcn_readfirstlane(s_begin), s_last, np, vm, ident, e, fl);
  if ((fl & MR_FOLD_ATE) && s_last == BN_ATE_STEPS && i < n && (st & BN254_ST_PENDING) && failed >= 0) status[i] = BN254_ST_NOT_IN_SUBGROUP;
}

__device__ __forceinline__ G1Proj rlc_g1_shfl_xor(const G1Proj& p, int mask) {
  G1Proj r;
#pragma unroll
  for (int l = 0; l < BN_NL; l++) { r.x.v[l] = __shfl_xor(p.x.v[l], mask); r.y.v[l] = __shfl_xor(p.y.v[l], mask); r.z.v[l] = __shfl_xor(p.z.v[l], mask); }
  BN_SETB(r.x, BN_VB(p.x), BN_LBD(p.x)); BN_SETB(r.y, BN_VB(p.y), BN_LBD(p.y)); BN_SETB(r.z, BN_VB(p.z), BN_LBD(p.z));
  return r;
}
// grid: one wavefront per group (n_groups * 64 lanes, rounded up to blocks of 256); the item of lane l of group g is 64 g + l
__global__ void __launch_bounds__(256, 2) k_pairing_rlc_group_sums(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int n_pairs, uint32_t shared_mask,
                                                                   const int32_t* __restrict__ prepared, int32_t* grp_ws, uint32_t n_groups, uint8_t* __restrict__ grp_status) {
  const uint32_t gl = blockIdx.x * 256u + threadIdx.x;
  const uint32_t g = gl >> 6, lane = gl & 63u, i = g * 64u + lane;
  const uint8_t st = i < n ? status[i] : (uint8_t)0;
  const bool pend = (st & BN254_ST_PENDING) != 0;
  const bool any = __builtin_amdgcn_ballot_w64(pend) != 0;
  const bool writer = lane == 0 && g < n_groups;
  if (!any) { if (writer) grp_status[g] = BN254_ST_ACCEPT; return; }      // (uniform over the wavefront)
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > PB_MAX_PAIRS ? PB_MAX_PAIRS : np);
  const uint32_t mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)shared_mask) & ((1u << np) - 1u);
  DevWs w(ws, n, i < n ? i : DEAD_LANE);
  DevWs wg(grp_ws, n_groups, writer ? g : DEAD_LANE);
  const uint32_t ident = pb_ident(w);
  uint32_t p_inf = 0;
  int t = 0;
#pragma unroll 1
  for (uint32_t m = mask; m; m &= m - 1, t++) {
    const int j = vp_first(m);
    G1Aff p; p.x = w.ld(vp_p(j)); p.y = w.ld(vp_p(j) + 1);
    const bool skip = !pend || ((ident >> (2 * j)) & 1u) != 0;
    G1Proj L = g1_from_affine(p);
    const G1Proj id = g1_identity();
    L.x = fp_select(skip, id.x, L.x); L.y = fp_select(skip, id.y, L.y); L.z = fp_select(skip, id.z, L.z);
    for (int x = 1; x < 64; x <<= 1) L = g1_add(L, rlc_g1_shfl_xor(L, x));
    const bool l_inf = g1_is_identity(L);
    G1Aff La = g1_to_affine(L);
    La.y = fp_select(l_inf, fp_one(), La.y);
    wg.st(vp_p(t), La.x); wg.st(vp_p(t) + 1, La.y);
    if (l_inf) p_inf |= 1u << t;
  }
  pb_rlc_group_finish(wg, mask, uni_ptr(prepared), p_inf);
  if (writer) grp_status[g] = BN254_ST_PENDING;
}

__device__ __forceinline__ Fp12 rlc_f12_shfl_xor(const Fp12& a, int mask) {
  Fp12 r;
#define RLC_SHFL(F) do { _Pragma("unroll") for (int l = 0; l < BN_NL; l++) r.F.v[l] = __shfl_xor(a.F.v[l], mask); BN_SETB(r.F, BN_VB(a.F), BN_LBD(a.F)); } while (0)
  RLC_SHFL(c0.c0.c0); RLC_SHFL(c0.c0.c1); RLC_SHFL(c0.c1.c0); RLC_SHFL(c0.c1.c1); RLC_SHFL(c0.c2.c0); RLC_SHFL(c0.c2.c1);
  RLC_SHFL(c1.c0.c0); RLC_SHFL(c1.c0.c1); RLC_SHFL(c1.c1.c0); RLC_SHFL(c1.c1.c1); RLC_SHFL(c1.c2.c0); RLC_SHFL(c1.c2.c1);
#undef RLC_SHFL
  return r;
}
__global__ void __launch_bounds__(256, 2) k_pairing_rlc_group_prod(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int32_t* grp_ws, uint32_t n_groups, int e_dst) {
  const uint32_t gl = blockIdx.x * 256u + threadIdx.x;
  const uint32_t g = gl >> 6, lane = gl & 63u, i = g * 64u + lane;
  const uint8_t st = i < n ? status[i] : (uint8_t)0;
  const bool pend = (st & BN254_ST_PENDING) != 0;
  if (__builtin_amdgcn_ballot_w64(pend) == 0) return;
  DevWs w(ws, n, i < n ? i : DEAD_LANE);
  DevWs wg(grp_ws, n_groups, (lane == 0 && g < n_groups) ? g : DEAD_LANE);
  Fp12 f = fp12_select(pend, pb_rlc_ld12(w, VE_F), fp12_one());
#pragma unroll 1
  for (int x = 1; x < 64; x <<= 1) f = pb_rlc_mul12(f, rlc_f12_shfl_xor(f, x));
  pb_rlc_st12(wg, __builtin_amdgcn_readfirstlane(e_dst), f);
}

}  // namespace bn254

using namespace bn254;
hipError_t bn254_launch_pairing_rlc_joint(const PairingRlcArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.n > (size_t)G16_MAX_LAUNCH || a.n_pairs < 1 || a.n_pairs > PB_MAX_PAIRS || (a.shared_mask >> a.n_pairs) != 0 || (a.shared_mask && (!a.prepared || ((uintptr_t)a.prepared & 3))) ||
      !a.ws || !a.status || !a.grp_ws || !a.grp_status || !a.one || (a.grp_form != PAIRING_FORM_LANES && a.grp_form != PAIRING_FORM_COOP))
    return hipErrorInvalidValue;
  const uint32_t nn = (uint32_t)a.n, all = (1u << a.n_pairs) - 1u, sh = a.shared_mask & all, var = all & ~sh;
  const size_t groups = (a.n + PB_RLC_GROUP - 1) / PB_RLC_GROUP;
  const uint32_t ng = (uint32_t)groups;
  const int n_sh = __builtin_popcount(sh);
  const unsigned grid = grid_for(a.n), ggrid = grid_for(groups * 64);
  hipError_t e;
  hipLaunchKernelGGL(k_pairing_rlc_weigh, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, a.n_pairs, a.weights, a.wkey);
  // the items: the Miller loop over the variable positions alone (the lane form at every size: the cooperative kernel has no mode that stops before the final
  // exponentiation).  No shared position: that is k_miller_run_var as it stands
  PairingLaunchArgs p;
  p.pairs = nullptr; p.item_stride = 0; p.one = a.one; p.out_gt = nullptr; p.skip_load = true;
  if (var && !sh) {
    p.n_pairs = a.n_pairs; p.n = a.n; p.ws = a.ws; p.status = a.status; p.form = PAIRING_FORM_LANES; p.miller_only = true;
    if ((e = bn254_launch_pairing_batch(p, s)) != hipSuccess) return e;
  } else if (var) {
    const MillerKinds& kinds = miller_step_table().packed;
    const int per = knob_run_steps_pairing_batch();
    for (int s0 = 0; s0 < BN_ATE_STEPS; s0 += per)
      hipLaunchKernelGGL(k_miller_run_sub, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, kinds, s0, s0 + per < BN_ATE_STEPS ? s0 + per : BN_ATE_STEPS, a.n_pairs, var, (int)VE_F,
                         (int)(MR_FOLD_INIT | MR_FOLD_ATE));
  }
  // the groups, behind the r-torsion tests: an item they decided is in neither the sums nor the product
  hipLaunchKernelGGL(k_pairing_rlc_group_sums, dim3(ggrid), dim3(256), 0, s, a.ws, nn, a.status, a.n_pairs, sh, a.prepared, a.grp_ws, ng, a.grp_status);
  if (var) hipLaunchKernelGGL(k_pairing_rlc_group_prod, dim3(ggrid), dim3(256), 0, s, a.ws, nn, a.status, a.grp_ws, ng, sh ? (int)PB_RLC_FG_ELEM : (int)VE_F);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the check of the groups: items of n_sh positions, every one of them shared
  int form = a.grp_form;
  if (form == PAIRING_FORM_COOP && groups > (size_t)COOP12_MAX_PROOFS) form = PAIRING_FORM_LANES;
  p.n = groups; p.ws = a.grp_ws; p.status = a.grp_status; p.miller_only = false; p.out_gt = a.out_grp_gt;
  if (!var) {
    p.n_pairs = n_sh; p.shared_mask = (1u << n_sh) - 1u; p.prepared = a.prepared; p.form = form;
    return bn254_launch_pairing_batch(p, s);
  }
  if (sh) {
    p.n_pairs = n_sh; p.shared_mask = (1u << n_sh) - 1u; p.prepared = a.prepared; p.form = PAIRING_FORM_LANES; p.miller_only = true;
    if ((e = bn254_launch_pairing_batch(p, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_f12_mul, dim3(grid_for(groups)), dim3(256), 0, s, a.grp_ws, ng, (const uint8_t*)a.grp_status, (int)VE_F, (int)VE_F, (int)PB_RLC_FG_ELEM, 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  p.n_pairs = 1; p.shared_mask = 0; p.prepared = nullptr; p.form = form; p.miller_only = false; p.skip_miller = true;
  return bn254_launch_pairing_batch(p, s);
}
