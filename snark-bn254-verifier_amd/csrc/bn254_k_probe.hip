// bn254_k_probe.hip -- what measures and what the value-level GPU tests look through: the VALU-peak kernel with its two measuring functions (bench.py prices its
// rooflines with them) and the k_dbg_* kernels with the bn254_launch_dbg_* launchers behind the bn254_dbg_* probes of bn254_capi_dbg.hip.  The operations the probes
// run are the product's own kernels (bn254_launch_ops.h); only the loads and stores of their operands are here.
#include <hip/hip_runtime.h>
#include "bn254_launch_ops.h"

namespace bn254 {
// Compiled twice (Makefile): the first object holds everything but the body of k_dbg_g2_subgroup; the second (-DBN_PLAIN_HALF -DBN_NO_CARRY_RIDE) holds only that kernel,
// which keeps the reassociated carry chains: with the carry ride it spills more (profiles/carry_chain_resources.txt).
#ifndef BN_PLAIN_HALF

// =====================================================================================================================
// the issue rate of the instruction every field product is made of, measured on THIS device: sixteen independent v_mad_u64_u32 chains per lane, two
// wavefronts per SIMD (tools/ubench_valu.hip: 1.92 ns per wavefront-instruction and SIMD on the box of profiles/r01_ubench_valu.txt = 35.1 T lane-mads/s;
// boxes of one pool differ by a few percent, so bench.py prices its rooflines with the rate of the box it runs on)
// =====================================================================================================================
#define VALU_PEAK_ITERS 16384
__global__ void __launch_bounds__(256) k_valu_peak(uint32_t* out, uint32_t seed, int iters) {
  const uint32_t tid = threadIdx.x + blockIdx.x * blockDim.x;
  const uint32_t a = seed * 2654435761u + tid, b = (seed ^ 0x9e3779b9u) + tid * 7u;
  uint64_t acc[16];
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = (uint64_t)(a + i) << 7 | (uint32_t)i;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int i = 0; i < 16; i++) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b) : "vcc");
  }
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) x ^= (uint32_t)acc[i] ^ (uint32_t)(acc[i] >> 32);
  out[tid] = x;
}

#endif
// =====================================================================================================================
// probes for the GPU parity tests
// =====================================================================================================================
__device__ __forceinline__ Fp probe_ld_fp(const uint8_t* p) {
  uint32_t w[8];
  words_from_be(w, p);
  return fp_from_words(w);
}
__device__ __forceinline__ void probe_st_fp(uint8_t* p, const Fp& a) {
  uint32_t w[8];
  fp_to_words(w, a);
  words_to_be(p, w);
}
#ifndef BN_PLAIN_HALF
__global__ void __launch_bounds__(256, 2) k_dbg_fp_mul(const uint8_t* a, const uint8_t* b, uint8_t* o, size_t n) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  probe_st_fp(o + 32 * i, fp_mul(probe_ld_fp(a + 32 * i), probe_ld_fp(b + 32 * i)));
}
// Fp12 / pairing probes: bytes (tower order) <-> workspace (k order); the operations themselves are the product's VM kernels
__global__ void __launch_bounds__(256, 2) k_dbg_load(int32_t* ws, uint32_t n, uint8_t* status, int e, const uint8_t* src, int kind) {
  // kind 0: Fp12 (384 B, tower order) -> element e; kind 1: G1 (64 B) -> VE_AX; kind 2: G2 (128 B, gnark order) -> VE_B; also marks the lane pending
  // kind 3: Fp12 as RAW DIGITS (12 x 9 int32, the twelve numbers in the tower order of kind 0, digit 0 first) -> element e, stored as given: the caller chooses the
  // representative (bn254_fp.h: Montgomery form, R = 2^261, balanced 29-bit digits) and answers for the operation's input contract; kind 4: G1 (64 B) -> e, e + 1
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  DevWs w(ws, n, i);
  if (kind == 0) {
    const int korder[6] = {0, 2, 4, 1, 3, 5};
    const uint8_t* p = src + 384 * (size_t)i;
    for (int t = 0; t < 6; t++) { w.st(e + 2 * korder[t], probe_ld_fp(p + 64 * t)); w.st(e + 2 * korder[t] + 1, probe_ld_fp(p + 64 * t + 32)); }
  } else if (kind == 3) {
    const int korder[6] = {0, 2, 4, 1, 3, 5};
    const int32_t* p = (const int32_t*)src + 12 * BN_NL * (size_t)i;
    for (int t = 0; t < 12; t++) { Fp a; for (int l = 0; l < BN_NL; l++) a.v[l] = p[t * BN_NL + l]; w.st(e + 2 * korder[t >> 1] + (t & 1), a); }
  } else if (kind == 4) {
    w.st(e, probe_ld_fp(src + 64 * (size_t)i)); w.st(e + 1, probe_ld_fp(src + 64 * (size_t)i + 32));
  } else if (kind == 1) {
    w.st(VE_AX, probe_ld_fp(src + 64 * (size_t)i)); w.st(VE_AY, probe_ld_fp(src + 64 * (size_t)i + 32));
  } else {
    const uint8_t* q = src + 128 * (size_t)i;
    w.st(VE_B + 1, probe_ld_fp(q)); w.st(VE_B, probe_ld_fp(q + 32)); w.st(VE_B + 3, probe_ld_fp(q + 64)); w.st(VE_B + 2, probe_ld_fp(q + 96));
  }
  status[i] = BN254_ST_PENDING;
}
__global__ void __launch_bounds__(256, 2) k_dbg_store(int32_t* ws, uint32_t n, int e, uint8_t* dst) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  DevWs w(ws, n, i);
  const int korder[6] = {0, 2, 4, 1, 3, 5};
  uint8_t* p = dst + 384 * (size_t)i;
  for (int t = 0; t < 6; t++) { probe_st_fp(p + 64 * t, w.ld(e + 2 * korder[t])); probe_st_fp(p + 64 * t + 32, w.ld(e + 2 * korder[t] + 1)); }
}
// the digits of element e as the workspace holds them (12 x 9 int32 per proof, the order of k_dbg_load's kind 3)
__global__ void __launch_bounds__(256, 2) k_dbg_store_raw(int32_t* ws, uint32_t n, int e, int32_t* dst) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  DevWs w(ws, n, i);
  const int korder[6] = {0, 2, 4, 1, 3, 5};
  int32_t* p = dst + 12 * BN_NL * (size_t)i;
  for (int t = 0; t < 12; t++) { const Fp a = w.ld(e + 2 * korder[t >> 1] + (t & 1)); for (int l = 0; l < BN_NL; l++) p[t * BN_NL + l] = a.v[l]; }
}
#endif
__global__ void __launch_bounds__(256, 2) k_dbg_g2_subgroup(const uint8_t* g2, uint8_t* o, size_t n)
#ifdef BN_PLAIN_HALF
{
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  G2Aff q; q.x.c1 = probe_ld_fp(g2 + 128 * i); q.x.c0 = probe_ld_fp(g2 + 128 * i + 32);
  q.y.c1 = probe_ld_fp(g2 + 128 * i + 64); q.y.c0 = probe_ld_fp(g2 + 128 * i + 96);
  o[i] = (g2_on_curve(q) && g2_in_subgroup(q)) ? 1 : 0;
}
#else
;
#endif
#ifndef BN_PLAIN_HALF
__global__ void __launch_bounds__(256, 2) k_dbg_g2_ate(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, uint8_t* o) {
  VM_KERNEL_PROLOGUE();
  bool ok = vm_g2_ate_check(w, VE_T, VE_B);
  if (i < n) o[i] = ok ? 1 : 0;
}

#endif
}  // namespace bn254
#ifndef BN_PLAIN_HALF

using namespace bn254;
// lane-level multiply-adds per second of the current device: the best launch of k_valu_peak at four wavefronts per SIMD, each about 2 ms long (a
// launch of 0.15 ms measured 20 % low: launch ramp and clocks), once `reps` launches in a row have not improved on it; 0 on failure
double bn254_measure_valu_peak(int reps) {
  hipDeviceProp_t p;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 0.0;
  const int grid = p.multiProcessorCount * 4;             // 256 threads = one wavefront on each SIMD of a CU; four blocks per CU
  uint32_t* out = nullptr;
  if (hipMalloc((void**)&out, (size_t)grid * 256 * 4) != hipSuccess) return 0.0;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipLaunchKernelGGL(k_valu_peak, dim3(grid), dim3(256), 0, nullptr, out, 1u, VALU_PEAK_ITERS);
  // The clocks of an idle GPU take tens of milliseconds of load to settle (the first five launches measured 29.7 T, the next five 32.2, then 33.2 against the
  // 34.8 T of a probe that runs for seconds): keep launching until the best has not improved for `reps` launches in a row, 200 launches (0.4 s) at most.
  float best = 1e30f;
  int since_best = 0;
  for (int r = 0; r < 200 && since_best < reps; r++) {
    (void)hipEventRecord(e0, nullptr);
    hipLaunchKernelGGL(k_valu_peak, dim3(grid), dim3(256), 0, nullptr, out, (uint32_t)(r + 2), VALU_PEAK_ITERS);
    (void)hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) != hipSuccess) { best = 1e30f; break; }
    float ms = 0.f;
    since_best++;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.f && ms < best * 0.998f) { best = ms; since_best = 0; }
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(out);
  if (best > 1e29f) return 0.0;
  return (double)grid * 256.0 * (double)VALU_PEAK_ITERS * 16.0 / ((double)best * 1e-3);
}
// The same kernel back to back for about `ms_target` milliseconds, timed as ONE interval: the rate the box sustains over the length of the path's long kernels
// (k_miller_run runs for 50 .. 100 ms) -- boxes whose best 2 ms launch agrees to 1 % differ by 3 % here (profiles/r05_box_variance.txt).
double bn254_measure_valu_sustained(double ms_target) {
  hipDeviceProp_t p;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 0.0;
  const int grid = p.multiProcessorCount * 4;
  uint32_t* out = nullptr;
  if (hipMalloc((void**)&out, (size_t)grid * 256 * 4) != hipSuccess) return 0.0;
  int launches = (int)(ms_target / 2.0);
  if (launches < 4) launches = 4;
  if (launches > 1000) launches = 1000;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, nullptr);
  for (int r = 0; r < launches; r++) hipLaunchKernelGGL(k_valu_peak, dim3(grid), dim3(256), 0, nullptr, out, (uint32_t)(r + 1), VALU_PEAK_ITERS);
  (void)hipEventRecord(e1, nullptr);
  float ms = 0.f;
  const bool ok = hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0.f;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(out);
  return ok ? (double)launches * grid * 256.0 * (double)VALU_PEAK_ITERS * 16.0 / ((double)ms * 1e-3) : 0.0;
}
hipError_t bn254_launch_dbg_fp_mul(const uint8_t* a, const uint8_t* b, uint8_t* o, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_dbg_fp_mul, dim3(grid_for(n)), dim3(256), 0, s, a, b, o, n);
  return hipGetLastError();
}
hipError_t bn254_launch_dbg_load(int32_t* ws, size_t n, uint8_t* status, int e, const void* src, int kind, hipStream_t s) {
  hipLaunchKernelGGL(k_dbg_load, dim3(grid_for(n)), dim3(256), 0, s, ws, (uint32_t)n, status, e, (const uint8_t*)src, kind);
  return hipGetLastError();
}
hipError_t bn254_launch_dbg_store(int32_t* ws, size_t n, int e, void* dst, int format, hipStream_t s) {
  if (format) hipLaunchKernelGGL(k_dbg_store_raw, dim3(grid_for(n)), dim3(256), 0, s, ws, (uint32_t)n, e, (int32_t*)dst);
  else hipLaunchKernelGGL(k_dbg_store, dim3(grid_for(n)), dim3(256), 0, s, ws, (uint32_t)n, e, (uint8_t*)dst);
  return hipGetLastError();
}
// op: 0 mul 1 sqr 2 inv 3 cyclo_sqr(easy part) 4 frob1 5 cyclo_sqr 6 frob2 7 frob3 8 mul by conj(b) 9 conj(a) * b (VE_CONJ on a).  status: n scratch bytes on the
// device.  in_format / out_format: 0 bytes (384 per value), 1 raw digits (k_dbg_load kind 3 / k_dbg_store_raw)
hipError_t bn254_launch_dbg_fp12_op_fmt(int op, const uint8_t* a, const uint8_t* b, uint8_t* o, size_t n, int32_t* ws, uint8_t* status, int in_format, int out_format, hipStream_t s) {
  unsigned g = grid_for(n);
  uint32_t nn = (uint32_t)n;
  LaunchOps ops{ws, nn, status, g, s, {nullptr, nullptr, nullptr}, nullptr};
  const int kind = in_format ? 3 : 0;
  hipLaunchKernelGGL(k_dbg_load, dim3(g), dim3(256), 0, s, ws, nn, status, (int)VE_F, a, kind);
  if (op == 0 || op == 8 || op == 9) {
    hipLaunchKernelGGL(k_dbg_load, dim3(g), dim3(256), 0, s, ws, nn, status, (int)VE_S1, b, kind);
    ops.f12_mul(VE_S0, op == 9 ? (VE_F | VE_CONJ) : VE_F, VE_S1, op == 8);
  }
  else if (op == 1) { ops.f12_sqr(VE_F); ops.f12_conj(VE_S0, VE_F); ops.f12_conj(VE_S0, VE_S0); }
  else if (op == 2) ops.f12_inv(VE_S0, VE_F);
  else if (op == 3) {
    ops.f12_inv(VE_S0, VE_F); ops.f12_conj(VE_S1, VE_F); ops.f12_mul(VE_S0, VE_S1, VE_S0); ops.f12_frob(VE_S1, VE_S0, 2);
    ops.f12_mul(VE_S0, VE_S1, VE_S0); ops.f12_cyclo_sqr(VE_S0, VE_S0);
  }
  else if (op == 5) ops.f12_cyclo_sqr(VE_S0, VE_F);
  else ops.f12_frob(VE_S0, VE_F, op == 6 ? 2 : op == 7 ? 3 : 1);
  (void)bn254_launch_dbg_store(ws, n, (int)VE_S0, o, out_format, s);
  return hipGetLastError();
}
// the two compares of the lane kernels on values a caller placed (bn254_dbg_verdict): form 0 k_g16_compare of VE_S0; form 1 k_f12_mul_verdict, the product's last
// launch dst = VE_S0 <- VE_S2 * VE_S0 compared as it is stored.  status: PENDING on entry, ACCEPT / REJECT on return
hipError_t bn254_launch_dbg_verdict(int form, int32_t* ws, size_t n, uint8_t* status, const int32_t* target, hipStream_t s) {
  unsigned grid = grid_for(n);
  uint32_t nn = (uint32_t)n;
  if (form == 0) hipLaunchKernelGGL(k_g16_compare, dim3(grid), dim3(256), 0, s, ws, nn, status, target, (int)BN254_ST_REJECT);
  else hipLaunchKernelGGL(k_f12_mul_verdict, dim3(grid), dim3(256), 0, s, ws, nn, status, (int)VE_S0, (int)VE_S2, (int)VE_S0, target, (int)BN254_ST_REJECT, (const uint32_t*)nullptr, status);
  return hipGetLastError();
}
// k_g16_prepare as a cooperative launch runs it, then k_coop12_miller_g16 in its store mode (a.target null): the GT value of every proof still pending
// after the loader is left in VE_S0, its status byte keeps PENDING; with a.target the kernel's own verdict, as bn254_launch_g16 launches it whatever BN254_COOP says.
// Keys with at most G16_WIDE_MSM_MIN_INPUTS inputs (L by the cooperative kernel itself)
hipError_t bn254_launch_dbg_coop12_g16(const G16LaunchArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_g16_prepare, dim3(grid_for(a.n)), dim3(256), 0, s, a.proofs, a.stride, a.inputs, a.n_public, (uint32_t)a.n, a.ws, a.status, a.msm_tab, a.k0, a.inputs_match_key, 1,
                     (const uint32_t*)nullptr, (uint8_t*)nullptr);
  return bn254_coop12_miller_g16(a.ws, a.status, a.n, a.gtab, a.dtab, a.inputs, a.n_public, a.inputs_match_key, a.msm_tab, a.k0, 0, a.target, s);
}
hipError_t bn254_launch_dbg_pairing(const uint8_t* g1, const uint8_t* g2, uint8_t* o, size_t n, int32_t* ws, uint8_t* status, hipStream_t s) {
  unsigned g = grid_for(n);
  uint32_t nn = (uint32_t)n;
  LaunchOps ops{ws, nn, status, g, s, {nullptr, nullptr, nullptr}, nullptr};
  hipLaunchKernelGGL(k_dbg_load, dim3(g), dim3(256), 0, s, ws, nn, status, 0, g1, 1);
  hipLaunchKernelGGL(k_dbg_load, dim3(g), dim3(256), 0, s, ws, nn, status, 0, g2, 2);
  hipLaunchKernelGGL(k_vm_init, dim3(g), dim3(256), 0, s, ws, nn, (const uint8_t*)status);
  vm_miller_program(ops, miller_step_table().kind, false);
  vm_final_exp_program(ops);
  hipLaunchKernelGGL(k_dbg_store, dim3(g), dim3(256), 0, s, ws, nn, (int)VE_S0, o);
  return hipGetLastError();
}
// r-torsion test through the product path: T from the Miller program (variable pair only, A = any G1 point), then the ate relation
hipError_t bn254_launch_dbg_g2_ate(const uint8_t* g1, const uint8_t* g2, uint8_t* o, size_t n, int32_t* ws, uint8_t* status, hipStream_t s) {
  unsigned g = grid_for(n);
  uint32_t nn = (uint32_t)n;
  LaunchOps ops{ws, nn, status, g, s, {nullptr, nullptr, nullptr}, nullptr};
  hipLaunchKernelGGL(k_dbg_load, dim3(g), dim3(256), 0, s, ws, nn, status, 0, g1, 1);
  hipLaunchKernelGGL(k_dbg_load, dim3(g), dim3(256), 0, s, ws, nn, status, 0, g2, 2);
  hipLaunchKernelGGL(k_vm_init, dim3(g), dim3(256), 0, s, ws, nn, (const uint8_t*)status);
  vm_miller_program(ops, miller_step_table().kind, false);
  hipLaunchKernelGGL(k_dbg_g2_ate, dim3(g), dim3(256), 0, s, ws, nn, (const uint8_t*)status, o);
  return hipGetLastError();
}
hipError_t bn254_launch_dbg_g2_subgroup(const uint8_t* g2, uint8_t* o, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_dbg_g2_subgroup, dim3(grid_for(n)), dim3(256), 0, s, g2, o, n);
  return hipGetLastError();
}
#endif
