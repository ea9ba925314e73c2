// bn254_k_miller.hip -- the Miller-loop step kernels of the large-batch (one proof per lane) Groth16 path: their own translation unit, because
// each instantiation is ~300 KB of straight-line code and the three of them dominate the library's compile time.
//   k_miller_step_dbl<DO_SQR>, k_miller_step_add: one whole step of the shared Miller loop (bn254_vm.h::vm_miller_step): [f <- f^2,] T <- 2T or
//   T + Q, f <- f * line_T(A) * line_gamma(L) * line_delta(C)   (replaces one iteration of bn's miller_loop_batch under groth16/verify.rs:73-77)
#include <cstdlib>
#include "bn254_devws.h"

namespace bn254 {

// the whole Miller step of the three pairs (bn254_vm.h::vm_miller_step): doubling steps (with the squaring of f, except the first)
// and addition steps as two kernels so that each carries only its own G2 formulas
template <bool DO_SQR>
__global__ void __launch_bounds__(256, 2) k_miller_step_dbl(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e_t, int e, int e_pa,
                                                            const int32_t* __restrict__ entry0, int e_p0, int inf_mask0,
                                                            const int32_t* __restrict__ entry1, int e_p1, int inf_mask1) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  FixedLine l0, l1;
  l0.m = uni_ld2(entry0); l0.c = uni_ld2(entry0 + 2 * BN_NL); l0.xc = uni_ld2(entry0 + 4 * BN_NL);
  l1.m = uni_ld2(entry1); l1.c = uni_ld2(entry1 + 2 * BN_NL); l1.xc = uni_ld2(entry1 + 4 * BN_NL);
  vm_miller_step<DO_SQR>(w, 0, e_t, 0, e, e_pa, l0, e_p0, (st & inf_mask0) != 0, l1, e_p1, (st & inf_mask1) != 0);
}
__global__ void __launch_bounds__(256, 2) k_miller_step_add(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int kind, int e_t, int e_b, int e, int e_pa,
                                                            const int32_t* __restrict__ entry0, int e_p0, int inf_mask0,
                                                            const int32_t* __restrict__ entry1, int e_p1, int inf_mask1) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  FixedLine l0, l1;
  l0.m = uni_ld2(entry0); l0.c = uni_ld2(entry0 + 2 * BN_NL); l0.xc = uni_ld2(entry0 + 4 * BN_NL);
  l1.m = uni_ld2(entry1); l1.c = uni_ld2(entry1 + 2 * BN_NL); l1.xc = uni_ld2(entry1 + 4 * BN_NL);
  int k = __builtin_amdgcn_readfirstlane(kind);
  vm_miller_step<false>(w, k < 1 ? 1 : k, e_t, e_b, e, e_pa, l0, e_p0, (st & inf_mask0) != 0, l1, e_p1, (st & inf_mask1) != 0);
}

// A RUN of steps in one launch (bn254_vm.h::vm_miller_run): steps [s_begin, s_end) of the loop -- by default the WHOLE loop.  f is loaded and stored
// once per run and travels in LDS + registers in between; the kind of a step and its line-table entries come from scalar loads indexed by the step.
// fold (MR_FOLD_INIT | MR_FOLD_ATE, bn254_vm.h): the launch that starts at step 0 sets f = 1 and T = (B, 1) itself (no k_vm_init before it), and the launch that
// ends the loop runs the r-torsion test of B on the point it has just produced and resolves the deferred statuses (no k_g16_subgroup after it): the one place
// where a run kernel WRITES the status byte it read in its prologue -- its own lane's, after its last use.
struct DevLines {
  const int32_t* tab0; const int32_t* tab1;
  __device__ __forceinline__ FixedLine get(int t, int s) const {
    const int32_t* e = (t == 0 ? tab0 : tab1) + (size_t)s * FIXED_LINE_DWORDS;
    FixedLine l; l.m = uni_ld2(e); l.c = uni_ld2(e + 2 * BN_NL); l.xc = uni_ld2(e + 4 * BN_NL);
    return l;
  }
};
struct DevKinds {   // the step table (88 entries, 0..4), two steps per byte, by value in the kernel arguments
  MillerKinds k;
  __device__ __forceinline__ int get(int s) const { return __builtin_amdgcn_readfirstlane((k.nib[s >> 1] >> ((s & 1) * 4)) & 15); }
};
__global__ void __launch_bounds__(256, 2) k_miller_run(int32_t* ws, uint32_t n, uint8_t* status, MillerKinds kinds, int s_begin, int s_end,
                                                       int e_t, int e_b, int e, int e_pa, const int32_t* __restrict__ tab0, int e_p0, int inf_mask0,
                                                       const int32_t* __restrict__ tab1, int e_p1, int inf_mask1, int fold, int inputs_match_key) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  DevLines lines{uni_ptr(tab0), uni_ptr(tab1)};
  DevKinds dk{kinds};
  const int s_last = __builtin_amdgcn_readfirstlane(s_end), fl = __builtin_amdgcn_readfirstlane(fold);
  const bool in_g2 = vm_miller_run(w, lines, dk, __builtin_amdgcn_readfirstlane(s_begin), s_last, e_t, e_b, e, e_pa, e_p0, (st & inf_mask0) != 0,
                                   e_p1, (st & inf_mask1) != 0, fl);
  if ((fl & MR_FOLD_ATE) && s_last == BN_ATE_STEPS && i < n && (st & BN254_ST_PENDING)) status[i] = g16_subgroup_status(st, in_g2, inputs_match_key);
}

// k_miller_run for a batch over many keys (bn254_keys.h): the same loop, the two line tables from the descriptor of the wavefront's key
__global__ void __launch_bounds__(256, 2) k_miller_run_keys(int32_t* ws, uint32_t n, uint8_t* status, MillerKinds kinds, int s_begin, int s_end,
                                                            int e_t, int e_b, int e, int e_pa, const G16KeyDesc* __restrict__ desc, uint32_t n_keys,
                                                            const uint32_t* __restrict__ granule_key, int e_p0, int inf_mask0, int e_p1, int inf_mask1, int fold) {
  __shared__ int32_t park_lds[72 * 256];
  if (((blockIdx.x * 256u + threadIdx.x) & ~63u) >= n) return;      // a wavefront past the launch's slots has no granule word
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  const KeyView kv = keys_view(desc, granule_key, i & ~63u, n_keys);
  DevLines lines{kv.gtab, kv.dtab};
  DevKinds dk{kinds};
  const int s_last = __builtin_amdgcn_readfirstlane(s_end), fl = __builtin_amdgcn_readfirstlane(fold);
  const bool in_g2 = vm_miller_run(w, lines, dk, __builtin_amdgcn_readfirstlane(s_begin), s_last, e_t, e_b, e, e_pa, e_p0, (st & inf_mask0) != 0,
                                   e_p1, (st & inf_mask1) != 0, fl);
  if ((fl & MR_FOLD_ATE) && s_last == BN_ATE_STEPS && i < n && (st & BN254_ST_PENDING)) status[i] = g16_subgroup_status(st, in_g2, kv.inputs_match);
}

// the loop of two table-driven pairs without a variable pair (bn254_vm.h::vm_miller_run_fixed2): the pairing check of a large PlonK batch
__global__ void __launch_bounds__(256, 2) k_miller_run_fixed2(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, MillerKinds kinds, int s_begin, int s_end, int e,
                                                              const int32_t* __restrict__ tab0, int e_p0, int inf_mask0, const int32_t* __restrict__ tab1, int e_p1, int inf_mask1) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  DevLines lines{uni_ptr(tab0), uni_ptr(tab1)};
  DevKinds dk{kinds};
  vm_miller_run_fixed2(w, lines, dk, __builtin_amdgcn_readfirstlane(s_begin), __builtin_amdgcn_readfirstlane(s_end), e, e_p0, (st & inf_mask0) != 0, e_p1, (st & inf_mask1) != 0);
}

// k_miller_run_fixed2 for a batch over many PlonK keys (bn254_keys.h): the same loop, the lines of the two KZG G2 points from the descriptor of the wavefront's key
__global__ void __launch_bounds__(256, 2) k_miller_run_fixed2_keys(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, MillerKinds kinds, int s_begin, int s_end, int e,
                                                                   const PlonkKeyDesc* __restrict__ desc, uint32_t n_keys, const uint32_t* __restrict__ granule_key,
                                                                   int e_p0, int inf_mask0, int e_p1, int inf_mask1) {
  __shared__ int32_t park_lds[72 * 256];
  if (((blockIdx.x * 256u + threadIdx.x) & ~63u) >= n) return;      // a wavefront past the launch's slots has no granule word
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  const PlonkKeyView kv = plonk_keys_view(desc, granule_key, i & ~63u, n_keys);
  DevLines lines{kv.tab0, kv.tab1};
  DevKinds dk{kinds};
  vm_miller_run_fixed2(w, lines, dk, __builtin_amdgcn_readfirstlane(s_begin), __builtin_amdgcn_readfirstlane(s_end), e, e_p0, (st & inf_mask0) != 0, e_p1, (st & inf_mask1) != 0);
}

}  // namespace bn254

using namespace bn254;
void bn254_launch_miller_run_fixed2_keys(const MillerKinds& kinds, int s_begin, int s_end, int32_t* ws, uint32_t n, const uint8_t* status, unsigned grid, hipStream_t s, int e,
                                         const PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, int ep0, int inf0, int ep1, int inf1) {
  hipLaunchKernelGGL(k_miller_run_fixed2_keys, dim3(grid), dim3(256), 0, s, ws, n, status, kinds, s_begin, s_end, e, desc, n_keys, granule_key, ep0, inf0, ep1, inf1);
}
void bn254_launch_miller_run_fixed2(const MillerKinds& kinds, int s_begin, int s_end, int32_t* ws, uint32_t n, const uint8_t* status, unsigned grid, hipStream_t s, int e,
                                    const int32_t* tab0, int ep0, int inf0, const int32_t* tab1, int ep1, int inf1) {
  hipLaunchKernelGGL(k_miller_run_fixed2, dim3(grid), dim3(256), 0, s, ws, n, status, kinds, s_begin, s_end, e, tab0, ep0, inf0, tab1, ep1, inf1);
}
void bn254_launch_miller_run(const MillerKinds& kinds, int s_begin, int s_end, int32_t* ws, uint32_t n, uint8_t* status, unsigned grid, hipStream_t s, int et, int eb,
                             int e, int epa, const int32_t* tab0, int ep0, int inf0, const int32_t* tab1, int ep1, int inf1, int fold, int inputs_match_key) {
  hipLaunchKernelGGL(k_miller_run, dim3(grid), dim3(256), 0, s, ws, n, status, kinds, s_begin, s_end, et, eb, e, epa, tab0, ep0, inf0, tab1, ep1, inf1, fold, inputs_match_key);
}
void bn254_launch_miller_run_keys(const MillerKinds& kinds, int s_begin, int s_end, int32_t* ws, uint32_t n, uint8_t* status, unsigned grid, hipStream_t s, int et, int eb,
                                  int e, int epa, const G16KeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, int ep0, int inf0, int ep1, int inf1, int fold) {
  hipLaunchKernelGGL(k_miller_run_keys, dim3(grid), dim3(256), 0, s, ws, n, status, kinds, s_begin, s_end, et, eb, e, epa, desc, n_keys, granule_key, ep0, inf0, ep1, inf1, fold);
}
void bn254_launch_miller_step(bool do_sqr, int kind, int32_t* ws, uint32_t n, const uint8_t* status, unsigned grid, hipStream_t s, int et, int eb, int e, int epa,
                              const int32_t* t0, int ep0, int inf0, const int32_t* t1, int ep1, int inf1) {
  if (kind == 0 && do_sqr) hipLaunchKernelGGL(k_miller_step_dbl<true>, dim3(grid), dim3(256), 0, s, ws, n, status, et, e, epa, t0, ep0, inf0, t1, ep1, inf1);
  else if (kind == 0) hipLaunchKernelGGL(k_miller_step_dbl<false>, dim3(grid), dim3(256), 0, s, ws, n, status, et, e, epa, t0, ep0, inf0, t1, ep1, inf1);
  else hipLaunchKernelGGL(k_miller_step_add, dim3(grid), dim3(256), 0, s, ws, n, status, kind, et, eb, e, epa, t0, ep0, inf0, t1, ep1, inf1);
}
