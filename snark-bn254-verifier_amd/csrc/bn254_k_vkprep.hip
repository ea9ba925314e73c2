// bn254_k_vkprep.hip -- the kernels of bn254_groth16_vk_prepare_batch (bn254_vkprep.h has the lane bodies, shared with the host probe): the once-per-key work of
// many verifying keys in one pass.
//   k_vkp_dec_g1    one lane per compressed G1 point of the pass (alpha, beta1, delta1 and every K point of every key: a wide key spreads over as many lanes)
//   k_vkp_dec_g2    one lane per compressed G2 point (beta, gamma, delta, the two points of the commitment key)
//   k_vkp_fold      one lane per key: did it load, the mode's negations, the arguments of the stages below
//   k_vkp_lines     one lane per (key, G2 argument): the 88-step line table, projective walk and one inversion
// e(alpha, b) of the pass's keys is the one-pair pairing program of the probes (bn254_launch_dbg_pairing), not a second Miller loop.
// The decode kernels run two Fp / Fp2 exponentiations and the walk 88 curve steps per lane, all on a handful of live field elements: the lanes are few (a pass of
// 4096 keys is 128 wavefronts of line tables) and long, so the blocks are one wavefront each -- they spread over the compute units instead of filling a few.
// Registers (gfx950, no scratch in any of them): dec_g1 84 VGPRs, dec_g2 194, fold 164, lines 256 -- one wavefront per SIMD, which is all a pass can offer a SIMD
// anyway (128 wavefronts for 1024 SIMDs); the walk keeps T, Q, the running product and a line live and is bound by the latency of its own chain.
#include <hip/hip_runtime.h>
#include "bn254_vkprep.h"

namespace bn254 {

__global__ void __launch_bounds__(64) k_vkp_dec_g1(const uint32_t* __restrict__ src, uint32_t n, int32_t* __restrict__ out, uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  vkp_dec_g1(src + (size_t)i * 8, out + (size_t)i * VKP_G1_DWORDS, ok + i);
}
__global__ void __launch_bounds__(64) k_vkp_dec_g2(const uint32_t* __restrict__ src, uint32_t n, int mode, int32_t* __restrict__ out, uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  vkp_dec_g2(src + (size_t)i * 16, mode, out + (size_t)i * VKP_G2_DWORDS, ok + i);
}
__global__ void __launch_bounds__(64) k_vkp_fold(const VkpKey* __restrict__ keys, uint32_t m, const uint8_t* __restrict__ ok1, const uint8_t* __restrict__ ok2,
                                                 const int32_t* __restrict__ g1pts, const int32_t* __restrict__ g2pts, int mode, uint8_t* __restrict__ key_ok,
                                                 int32_t* __restrict__ targ, int32_t* __restrict__ barg, uint8_t* __restrict__ pair_g1, uint8_t* __restrict__ pair_g2) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= m) return;
  vkp_fold(j, keys, ok1, ok2, g1pts, g2pts, mode, key_ok, targ, barg, pair_g1, pair_g2);
}
__global__ void __launch_bounds__(64) k_vkp_lines(const int32_t* __restrict__ targ, uint32_t n, int32_t* __restrict__ tabs, uint8_t* __restrict__ tab_ok) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const G2Aff q = vkp_get_g2(targ + (size_t)i * VKP_G2_DWORDS);
  tab_ok[i] = vkp_line_table(tabs + (size_t)i * VKP_TAB_DWORDS, q) ? 1 : 0;
}

}  // namespace bn254

using namespace bn254;
static inline unsigned vkp_grid(uint32_t n) { return (n + 63u) / 64u; }

hipError_t bn254_launch_vkprep(const VkpLaunchArgs& a, hipStream_t s, hipEvent_t* ev) {
  if (a.m == 0) return hipSuccess;
  const uint32_t n_g2 = a.m * VKP_G2_PER_KEY;
  if (ev) (void)hipEventRecord(ev[0], s);
  if (a.n_g1) hipLaunchKernelGGL(k_vkp_dec_g1, dim3(vkp_grid(a.n_g1)), dim3(64), 0, s, a.g1_src, a.n_g1, a.g1pts, a.ok1);
  if (ev) (void)hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(k_vkp_dec_g2, dim3(vkp_grid(n_g2)), dim3(64), 0, s, a.g2_src, n_g2, a.mode, a.g2pts, a.ok2);
  if (ev) (void)hipEventRecord(ev[2], s);
  hipLaunchKernelGGL(k_vkp_fold, dim3(vkp_grid(a.m)), dim3(64), 0, s, a.keys, a.m, (const uint8_t*)a.ok1, (const uint8_t*)a.ok2, (const int32_t*)a.g1pts, (const int32_t*)a.g2pts,
                     a.mode, a.key_ok, a.targ, a.barg, a.pair_g1, a.pair_g2);
  if (ev) (void)hipEventRecord(ev[3], s);
  hipLaunchKernelGGL(k_vkp_lines, dim3(vkp_grid(2 * a.m)), dim3(64), 0, s, (const int32_t*)a.targ, 2 * a.m, a.tabs, a.tab_ok);
  if (ev) (void)hipEventRecord(ev[4], s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = bn254_launch_dbg_pairing(a.pair_g1, a.pair_g2, a.gt, a.m, a.ws, a.ws_status, s);
  if (ev) (void)hipEventRecord(ev[5], s);
  return e;
}
