// bn254_k_g1msm.hip -- batch G1 multi-scalar multiplication over caller records (include/bn254_verify.h, bn254_g1_msm_batch; bn254_g1msm.h): the kernels in front of
// and behind the G1 walk, one item per lane.
//   k_g1_msm_load    the item's record -> the loader's status byte and the TERM records k_g1_msm_rows walks (bn254_g1msm.h::g1msm_load_item: strict scalars, range and
//                    curve checks in record order, scalars modulo r, glv_decompose for the variable terms, the canonical scalar words for the shared positions)
//   k_g1_msm_store   behind k_g1_sum_affine (words form): the sum and its identity flag -> 64 big-endian bytes and the final status byte
// The walk itself is bn254_k_msm.hip (k_g1_msm_rows with the handle's window tables, k_g1_sum_affine to canonical words).
#include <hip/hip_runtime.h>
#include "bn254_devws.h"
#include "bn254_g1msm.h"

namespace bn254 {

// the shape counts are the call's: uniform over the launch, held in scalar registers (the term loops run in step)
__global__ void __launch_bounds__(256, 2) k_g1_msm_load(const uint8_t* __restrict__ items, size_t stride, uint32_t n, int n_var, int n_unit, int n_shared, uint32_t dead_bases,
                                                        int strict, uint8_t* __restrict__ status, int32_t* __restrict__ terms, uint8_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int nv = __builtin_amdgcn_readfirstlane(n_var), nu = __builtin_amdgcn_readfirstlane(n_unit), ns = __builtin_amdgcn_readfirstlane(n_shared);
  const int n_terms = nv + nu + ns;
  const bool aligned = ((((uintptr_t)items) | stride) & 3) == 0;
  status[i] = (uint8_t)g1msm_load_item(items + (size_t)i * stride, aligned, nv, nu, ns, (uint32_t)__builtin_amdgcn_readfirstlane((int)dead_bases), strict != 0,
                                       terms + (size_t)i * (size_t)n_terms * MSM_TERM_DWORDS, flags + (size_t)i * (size_t)n_terms);
}

// 64 bytes per lane at a 64-byte pitch: every lane writes whole cache-line halves of its own
__global__ void __launch_bounds__(256, 2) k_g1_msm_store(const uint32_t* __restrict__ words, const uint8_t* __restrict__ inf, const uint8_t* __restrict__ st, uint32_t n,
                                                         uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t w[16];
  const uint4* q = (const uint4*)(words + (size_t)i * 16);
#pragma unroll
  for (int k = 0; k < 4; k++) { const uint4 v = q[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
  g1msm_store_item(out + 64 * (size_t)i, status + i, st[i], w, inf[i] != 0, (((uintptr_t)out) & 3) == 0);
}

}  // namespace bn254

using namespace bn254;
hipError_t bn254_launch_g1msm_load(const G1MsmLoadArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.n > G1MSM_MAX_PASS || a.n_var < 0 || a.n_unit < 0 || a.n_shared < 0 || !g1msm_shape_ok((size_t)a.n_var, (size_t)a.n_unit, (size_t)a.n_shared) || !a.items ||
      a.stride < G1MSM_ITEM_LEN(a.n_var, a.n_unit, a.n_shared) || !a.status || !a.terms || !a.flags)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_g1_msm_load, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.items, a.stride, (uint32_t)a.n, a.n_var, a.n_unit, a.n_shared, a.dead_bases,
                     a.strict ? 1 : 0, a.status, a.terms, a.flags);
  return hipGetLastError();
}
hipError_t bn254_launch_g1msm_store(const uint32_t* words, const uint8_t* inf, const uint8_t* st, size_t n, uint8_t* out, uint8_t* status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > G1MSM_MAX_PASS || !words || ((uintptr_t)words & 15) || !inf || !st || !out || !status) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_g1_msm_store, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, words, inf, st, (uint32_t)n, out, status);
  return hipGetLastError();
}
