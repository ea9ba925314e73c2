// bn254_k_pairing.hip -- the batch pairing product over caller-supplied pairs (bn::pairing_batch of groth16/verify.rs:73-77 and plonk/kzg.rs:175-187, without a key;
// include/bn254_verify.h, bn254_pairing_check_batch): one item of up to eight (G1, G2) pairs per lane.  Its own translation unit for the reason bn254_k_miller.hip gives:
// a run kernel is ~300 KB of straight-line code.
//   k_pairing_load     the item's records -> points, identity bits and the status byte (bn254_pairing_batch.h::pb_load_item: the range and on-curve checks)
//   k_miller_run_var   steps [s_begin, s_end) of the optimal-ate loop for the item's pairs, f in flight (bn254_vm.h::vm_miller_run_var); the run that ends the loop
//                      decides the r-torsion tests and writes the status of an item that failed one
//   k_pairing_load_shared, k_miller_run_mix   the same two for items whose G2 point of some positions is shared by the whole batch and prepared
//                      (bn254_g2_prepare: the affine point and its 88 lines): packed records, table-driven line products for the shared positions
//   k_pairing_store    the store tail: VE_S0 in the 384-byte format 0 of bn254_dbg_pairing
// then vm_final_exp_program through LaunchOps and k_g16_compare against 1 in GT (the kernels of bn254_kernels.hip).
// A small launch (bn254_g16_plan.h::pairing_form) takes the cooperative form instead: k_pairing_load, then bn254_coop12.hip::k_coop12_miller_pairs, twelve lanes per
// item, and -- unless the verdict alone is wanted, which that kernel writes itself -- the same tails.  The choice is made here, in bn254_launch_pairing_batch.
#include <hip/hip_runtime.h>
#include "bn254_launch_ops.h"
#include "bn254_g16_plan.h"
#include "bn254_pairing_batch.h"

namespace bn254 {

__global__ void __launch_bounds__(256, 2) k_pairing_load(const uint8_t* __restrict__ pairs, size_t item_stride, int n_pairs, uint32_t n, int32_t* ws, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  DevWs w(ws, n, i);
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > PB_MAX_PAIRS ? PB_MAX_PAIRS : np);
  const bool aligned = ((((uintptr_t)pairs) | item_stride) & 3) == 0;
  status[i] = (uint8_t)pb_load_item(w, pairs + (size_t)i * item_stride, np, aligned);
}

struct PairKinds {   // the step table (88 entries, 0..4), two steps per byte, by value in the kernel arguments
  MillerKinds k;
  __device__ __forceinline__ int get(int s) const { return __builtin_amdgcn_readfirstlane((k.nib[s >> 1] >> ((s & 1) * 4)) & 15); }
};
__global__ void __launch_bounds__(256, 2) k_miller_run_var(int32_t* ws, uint32_t n, uint8_t* status, MillerKinds kinds, int s_begin, int s_end, int n_pairs, int e, int fold) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  PairKinds pk{kinds};
  const int s_last = __builtin_amdgcn_readfirstlane(s_end), fl = __builtin_amdgcn_readfirstlane(fold);
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > PB_MAX_PAIRS ? PB_MAX_PAIRS : np);
  const uint32_t ident = pb_ident(w);
  const int failed = vm_miller_run_var(w, pk, __builtin_amdgcn_readfirstlane(s_begin), s_last, np, ident, e, fl);
  if ((fl & MR_FOLD_ATE) && s_last == BN_ATE_STEPS && i < n && (st & BN254_ST_PENDING) && failed >= 0) status[i] = BN254_ST_NOT_IN_SUBGROUP;
}

// ---- items with shared, prepared G2 points (bn254_pairing_check_batch_shared) ---------------------------------------------------------------------------------------
// k_pairing_load_shared: the PACKED record of an item (a shared position holds its G1 point alone) through the checks of k_pairing_load; the affine point and the
// identity flag of a shared position come from its prepared record, so the workspace is what k_pairing_load leaves for the expanded item.  The header words of every
// record are read first, at wave-uniform addresses: a record of another magic word or layout version makes every item MALFORMED, so that no run kernel sees a pending
// item and no table is ever read.
__global__ void __launch_bounds__(256, 2) k_pairing_load_shared(const uint8_t* __restrict__ items, size_t item_stride, int n_pairs, uint32_t shared_mask, const int32_t* __restrict__ prepared,
                                                               uint32_t n, int32_t* ws, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  DevWs w(ws, n, i);
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > PB_MAX_PAIRS ? PB_MAX_PAIRS : np);
  const uint32_t mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)shared_mask) & ((1u << np) - 1u);
  const int32_t* prep = uni_ptr(prepared);
  if (!pb_records_ok(prep, mask)) { status[i] = BN254_ST_MALFORMED; return; }
  const bool aligned = ((((uintptr_t)items) | item_stride) & 3) == 0;
  status[i] = (uint8_t)pb_load_item_shared(w, items + (size_t)i * item_stride, np, mask, prep, aligned);
}

// k_miller_run_mix: steps [s_begin, s_end) for an item whose positions are variable or shared (bn254_vm.h::vm_miller_run_mix).  The mask is a kernel argument, so which
// positions are shared is launch-uniform; the lines of a shared position come from its record's table by scalar loads indexed by the step (DevLines' pattern).  With
// every position shared the launcher takes the instantiation VAR = false, which holds no G2 arithmetic and no r-torsion test.
struct PrepLines {
  const int32_t* prepared;
  __device__ __forceinline__ FixedLine get(int t, int s) const {
    const int32_t* e = prepared + (size_t)t * PB_PREP_DWORDS + (PB_PREP_HDR_DWORDS + PB_PREP_POINT_DWORDS) + (size_t)s * FIXED_LINE_DWORDS;
    FixedLine l; l.m = uni_ld2(e); l.c = uni_ld2(e + 2 * BN_NL); l.xc = uni_ld2(e + 4 * BN_NL);
    return l;
  }
};
template <bool VAR>
__global__ void __launch_bounds__(256, 2) k_miller_run_mix(int32_t* ws, uint32_t n, uint8_t* status, MillerKinds kinds, int s_begin, int s_end, int n_pairs, uint32_t shared_mask,
                                                          const int32_t* __restrict__ prepared, int e, int fold) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  PairKinds pk{kinds};
  const int s_last = __builtin_amdgcn_readfirstlane(s_end), fl = __builtin_amdgcn_readfirstlane(fold);
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > PB_MAX_PAIRS ? PB_MAX_PAIRS : np);
  const uint32_t all = (1u << np) - 1u, mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)shared_mask) & all;
  PrepLines lines{uni_ptr(prepared)};
  const uint32_t ident = pb_ident(w);
  const int failed = vm_miller_run_mix<VAR>(w, lines, pk, __builtin_amdgcn_readfirstlane(s_begin), s_last, VAR ? all & ~mask : 0u, VAR ? mask : all, ident, e, fl);
  if (VAR && (fl & MR_FOLD_ATE) && s_last == BN_ATE_STEPS && i < n && (st & BN254_ST_PENDING) && failed >= 0) status[i] = BN254_ST_NOT_IN_SUBGROUP;
}

// finalize: the store is the launch's last word on a pending item -- its status becomes ACCEPT ("out_gt holds the value")
__global__ void __launch_bounds__(256, 2) k_pairing_store(int32_t* ws, uint32_t n, uint8_t* status, uint8_t* __restrict__ out_gt, int finalize) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !(status[i] & BN254_ST_PENDING)) return;
  DevWs w(ws, n, i);
  const int korder[6] = {0, 2, 4, 1, 3, 5};
  uint8_t* p = out_gt + 384 * (size_t)i;
  for (int t = 0; t < 6; t++)
    for (int h = 0; h < 2; h++) { uint32_t v[8]; fp_to_words(v, w.ld(VE_S0 + 2 * korder[t] + h)); words_to_be(p + 64 * t + 32 * h, v); }
  if (finalize) status[i] = BN254_ST_ACCEPT;
}

}  // namespace bn254

using namespace bn254;
hipError_t bn254_launch_pairing_batch(const PairingLaunchArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.n > (size_t)G16_MAX_LAUNCH || a.n_pairs < 1 || a.n_pairs > PB_MAX_PAIRS || (!a.one && !a.out_gt)) return hipErrorInvalidValue;
  if ((a.shared_mask >> a.n_pairs) != 0 || (a.shared_mask && (!a.prepared || ((uintptr_t)a.prepared & 3))) || (!a.skip_load && a.item_stride < pb_item_len(a.n_pairs, a.shared_mask))) return hipErrorInvalidValue;
  const unsigned grid = grid_for(a.n);
  const uint32_t nn = (uint32_t)a.n;
  const int form = a.form != PAIRING_FORM_PLAN ? a.form : pairing_form((size_t)a.n_pairs, a.n, (size_t)PAIRING_COOP_MAX_DEFAULT, knob_coop_on());
  if (form != PAIRING_FORM_LANES && (form != PAIRING_FORM_COOP || a.n > (size_t)COOP12_MAX_PROOFS)) return hipErrorInvalidValue;
  // shared_mask == 0 is the path of the all-variable entry, kernel for kernel; skip_load: the caller's own loader has filled the workspace and the status bytes
  if (a.skip_load) {}
  else if (a.shared_mask) hipLaunchKernelGGL(k_pairing_load_shared, dim3(grid), dim3(256), 0, s, a.pairs, a.item_stride, a.n_pairs, (uint32_t)a.shared_mask, a.prepared, nn, a.ws, a.status);
  else hipLaunchKernelGGL(k_pairing_load, dim3(grid), dim3(256), 0, s, a.pairs, a.item_stride, a.n_pairs, nn, a.ws, a.status);
  if (a.load_only) return hipGetLastError();
  if (a.miller_only && (form != PAIRING_FORM_LANES || a.skip_miller)) return hipErrorInvalidValue;
  if (a.skip_miller && form == PAIRING_FORM_COOP) {      // VE_F -> VE_S0 in one launch, then the tails of the lane form
    const hipError_t e = bn254_coop12_final_exp(a.ws, a.status, a.n, s);
    if (e != hipSuccess) return e;
    if (a.out_gt) hipLaunchKernelGGL(k_pairing_store, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, a.out_gt, a.one ? 0 : 1);
    if (a.one) hipLaunchKernelGGL(k_g16_compare, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, a.one, (int)BN254_ST_REJECT);
    return hipGetLastError();
  }
  if (form == PAIRING_FORM_COOP) {
    // twelve lanes per item (after k_pairing_load_shared as well: the shared points are in the workspace as if they had come from the item, and the form has no use
    // for the tables): the Miller loop, the r-torsion tests and the final exponentiation in one launch -- with the verdict when that is all the caller wants,
    // otherwise the GT value to VE_S0 and the tails of the lane form
    const bool fused = a.one && !a.out_gt;
    const hipError_t e = bn254_coop12_miller_pairs(a.ws, a.status, a.n, a.n_pairs, fused ? a.one : nullptr, s);
    if (e != hipSuccess || fused) return e;
    if (a.out_gt) hipLaunchKernelGGL(k_pairing_store, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, a.out_gt, a.one ? 0 : 1);
    if (a.one) hipLaunchKernelGGL(k_g16_compare, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, a.one, (int)BN254_ST_REJECT);
    return hipGetLastError();
  }
  const MillerKinds& kinds = miller_step_table().packed;
  const int per = knob_run_steps_pairing_batch();
  for (int s0 = 0; s0 < BN_ATE_STEPS && !a.skip_miller; s0 += per)
    if (a.shared_mask)
      hipLaunchKernelGGL(a.shared_mask == (1u << a.n_pairs) - 1u ? k_miller_run_mix<false> : k_miller_run_mix<true>, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, kinds, s0, s0 + per < BN_ATE_STEPS ? s0 + per : BN_ATE_STEPS, a.n_pairs, (uint32_t)a.shared_mask,
                         a.prepared, (int)VE_F, (int)(MR_FOLD_INIT | MR_FOLD_ATE));
    else
      hipLaunchKernelGGL(k_miller_run_var, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, kinds, s0, s0 + per < BN_ATE_STEPS ? s0 + per : BN_ATE_STEPS, a.n_pairs, (int)VE_F,
                       (int)(MR_FOLD_INIT | MR_FOLD_ATE));
  if (a.miller_only) return hipGetLastError();
  LaunchOps ops{a.ws, nn, a.status, grid, s, {nullptr, nullptr, nullptr}, nullptr};
  vm_final_exp_program(ops);
  if (a.out_gt) hipLaunchKernelGGL(k_pairing_store, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, a.out_gt, a.one ? 0 : 1);
  if (a.one) hipLaunchKernelGGL(k_g16_compare, dim3(grid), dim3(256), 0, s, a.ws, nn, a.status, a.one, (int)BN254_ST_REJECT);
  return hipGetLastError();
}
