// bn254_k_plonk.hip -- the per-proof HOST stages of the PlonK verifier as device kernels, one proof per lane (round 3).
//
// plonk/verify.rs:46-284 and kzg.rs:46-190 up to the group operations -- proof parsing and curve checks (plonk/converter.rs:121-178), the four
// Fiat-Shamir challenges and the folding challenge (transcript.rs:15-108: SHA-256), the BSB22 hash-to-field (hash_to_field.rs:45-97), the scalar-field
// arithmetic of the linearisation, the GLV split of every MSM scalar -- are the SAME source as the host path: bn254_plonk.hpp compiled with
// BN254_PLONK_DEVICE_TU, which makes its functions __host__ __device__.  A batch then stays on the GPU between its one H2D copy (proofs, inputs) and
// its one D2H copy (status bytes): no device -> host -> device round trip between the two MSM stages, no host threads.
//   k_plonk_stage1: transcripts gamma / beta / alpha / zeta, opening check, the T1 terms of the linearised-polynomial digest, lambda (ChaCha20)
//   k_plonk_stage2: folding transcript over the digest (the first MSM's result, read from device memory), the T2 + 2 terms of the KZG check
// A lane runs ~250 k instructions on its own; 4096 proofs are 64 wavefronts, so the launches are latency-bound (one wavefront per SIMD, 64-thread
// workgroups so that they spread over the chip).
#define BN254_PLONK_DEVICE_TU 1
#include <hip/hip_runtime.h>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>
#include "bn254_plonk.hpp"
#include "bn254_rlc.h"
#include "bn254_keys.h"

using namespace bn254host;

namespace bn254 {

// Dynamic LDS of both kernels (bn254_plonk.hpp::pl_lane_lds): [0] u32 lane stride | per lane: 64-byte SHA block, the proof's bytes, its public inputs.
// The 64 proofs of a workgroup are copied in cooperatively -- one proof at a time, the lanes on consecutive dwords -- so that the byte-wise reads of
// the parser and of the transcripts hit LDS instead of each lane walking its own 900 bytes of global memory.  Returns the lane's proof pointer.
#define PL_STAGE_MAX_PROOF 1664      // 516 + 32 x 16 claimed values + 100 + 64 x 8 commitments: the most the parser reads
#define PL_STAGE_MAX_INPUT 256       // public inputs staged up to 8; beyond that they are read from global memory
// rows [first, first + 64) of a byte matrix (row stride src_stride, `bytes` of each row, everything a multiple of 4) -> the lanes' LDS slots (row j at dst0 + j * lane_stride)
__device__ __forceinline__ void pl_stage_rows(uint8_t* dst0, uint32_t lane_stride, const uint8_t* __restrict__ src, size_t src_stride, size_t bytes, uint32_t first, uint32_t n, size_t nt) {
  for (uint32_t j0 = 0; j0 < 64; j0 += 16) {
    if (first + j0 >= n) break;
    for (size_t off = 4 * (size_t)threadIdx.x; off < bytes; off += 4 * nt) {
      uint32_t v[16];
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) { const uint32_t rec = first + j0 + u; v[u] = rec < n ? *(const uint32_t*)(src + (size_t)rec * src_stride + off) : 0u; }
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) *(uint32_t*)(dst0 + (size_t)(j0 + u) * lane_stride + off) = v[u];
    }
  }
}
// in_stride: bytes between the input rows of consecutive records (32 n_public in a single-key batch; the row width of the widest key in a batch over many keys)
__device__ __forceinline__ const uint8_t* pl_stage_lds_rows(const uint8_t* __restrict__ proofs, size_t stride, const uint8_t* __restrict__ inputs, size_t in_stride, size_t n_public,
                                                          uint32_t n, uint32_t lane_stride, const uint8_t** lane_inputs) {
  extern __shared__ uint8_t pl_dyn_lds[];
  // bn254_plonk.hpp::pl_lane_lds addresses the lanes' slots by LDS OFFSET (it may be compiled out of line, where the array has no name): that is only right while
  // this array starts at offset 0, i.e. while neither the kernels nor anything the compiler places (a promoted alloca, a static __shared__ of an inlined callee)
  // owns LDS in front of it.  If that ever changes the transcripts would hash foreign bytes: stop the launch instead.
  if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)pl_dyn_lds != 0u) __builtin_trap();
  if (threadIdx.x == 0) *(uint32_t*)pl_dyn_lds = lane_stride;
  const size_t pbytes = stride < PL_STAGE_MAX_PROOF ? stride : PL_STAGE_MAX_PROOF;
  const size_t ibytes = n_public * 32 <= PL_STAGE_MAX_INPUT ? n_public * 32 : 0;
  const uint32_t first = blockIdx.x * 64u;
  const bool aligned = (((uintptr_t)proofs | stride | (uintptr_t)inputs | in_stride) & 3) == 0;
  const size_t nt = blockDim.x;             // 64 (k_plonk_stage2) or 128 (k_plonk_stage1: chain + helper wavefront, the same 64 proofs)
  if (aligned) {
    // SIXTEEN records per step: a thread's sixteen loads are in flight together (one record at a time was 64 dependent round trips to HBM: 85 us of a 390 us launch)
    pl_stage_rows(pl_dyn_lds + 16 + 64, lane_stride, proofs, stride, pbytes, first, n, nt);
    if (ibytes) pl_stage_rows(pl_dyn_lds + 16 + 64 + ((pbytes + 3) & ~(size_t)3), lane_stride, inputs, in_stride, ibytes, first, n, nt);
  } else {
    for (uint32_t j = 0; j < 64; j++) {
      const uint32_t rec = first + j;
      if (rec >= n) break;
      uint8_t* dst = pl_dyn_lds + 16 + (size_t)j * lane_stride + 64;
      const uint8_t* src = proofs + (size_t)rec * stride;
      const uint8_t* isrc = inputs + (size_t)rec * in_stride;
      for (size_t off = threadIdx.x; off < pbytes; off += nt) dst[off] = src[off];
      for (size_t off = threadIdx.x; off < ibytes; off += nt) dst[((pbytes + 3) & ~(size_t)3) + off] = isrc[off];
    }
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = first + lane;
  const uint8_t* mine = pl_dyn_lds + 16 + (size_t)lane * lane_stride + 64;
  *lane_inputs = ibytes ? mine + ((pbytes + 3) & ~(size_t)3) : inputs + (size_t)(i < n ? i : 0) * in_stride;
  return mine;
}
__device__ __forceinline__ const uint8_t* pl_stage_lds(const uint8_t* __restrict__ proofs, size_t stride, const uint8_t* __restrict__ inputs, size_t n_public, uint32_t n,
                                                     uint32_t lane_stride, const uint8_t** lane_inputs) {
  return pl_stage_lds_rows(proofs, stride, inputs, n_public * 32, n_public, n, lane_stride, lane_inputs);
}
static uint32_t pl_lane_stride(size_t stride, size_t n_public) {
  const size_t pbytes = stride < PL_STAGE_MAX_PROOF ? stride : PL_STAGE_MAX_PROOF;
  const size_t ibytes = n_public * 32 <= PL_STAGE_MAX_INPUT ? n_public * 32 : 0;
  size_t dw = (64 + ((pbytes + 3) & ~(size_t)3) + ibytes) / 4;
  if (!(dw & 1)) dw++;                 // an odd number of dwords per lane: the lanes' same-offset accesses fall on different banks
  return (uint32_t)(dw * 4);
}

// Two lanes per proof, in two wavefronts of a 128-thread workgroup (round 4).  A lane's chain was 478 us at 4096 proofs -- one wavefront per SIMD, nothing to
// hide latency behind -- of which 172 us do not depend on the transcripts: the curve checks and digit conversions of the nine points (parse_plonk_proof), the BSB22
// hash_to_field, lambda.  Wavefront 1 (lanes 64..127) does those for the same 64 proofs while wavefront 0 runs transcripts -> zeta^n -> denominators -> inversion
// from the proof's bytes and its layout alone; they meet at ONE barrier (the parsed proof and the hashes travel through work[i], the status precedence is the
// reference's: a loader error of any point beats everything the chain lane found), then wavefront 0 finishes (public-input sum, opening check, terms).
// The stage behind the staging is pl_stage1_body, below the kernel: my_proof / my_inputs are the lane's record (stride: the length the parser is told) and input
// row.  One body for k_plonk_stage1 and k_plonk_stage1_keys, which differ in where the key and the input width come from
__device__ __forceinline__ void pl_stage1_body(const PlonkKey* __restrict__ key, const uint8_t* my_proof, const uint8_t* my_inputs, size_t stride, size_t n_public, uint32_t n,
                                               const ChaChaKey& lam_key, PlonkWork* work, MsmTerm* terms, uint8_t* flags, int T1);
__global__ void __launch_bounds__(128) k_plonk_stage1(const PlonkKey* __restrict__ key, const uint8_t* __restrict__ proofs, size_t stride, const uint8_t* __restrict__ inputs,
                                                      size_t n_public, uint32_t n, ChaChaKey lam_key, PlonkWork* work, MsmTerm* terms,
                                                      uint8_t* flags, int T1, uint32_t lane_stride) {
  const uint8_t* my_inputs;
  const uint8_t* my_proof = pl_stage_lds(proofs, stride, inputs, n_public, n, lane_stride, &my_inputs);
  pl_stage1_body(key, my_proof, my_inputs, stride, n_public, n, lam_key, work, terms, flags, T1);
}
__device__ __forceinline__ void pl_stage1_body(const PlonkKey* __restrict__ key, const uint8_t* my_proof, const uint8_t* my_inputs, size_t stride, size_t n_public, uint32_t n,
                                               const ChaChaKey& lam_key, PlonkWork* work, MsmTerm* terms, uint8_t* flags, int T1) {
  const bool helper = threadIdx.x >= 64u;
  const uint32_t i = blockIdx.x * 64u + (threadIdx.x & 63u);
  const bool live = i < n;                      // no early return: every lane reaches the barrier
  const FrCtx& F = fr_ctx();
  PlonkWork& wk = work[live ? i : 0];
  MsmTerm* t = terms + (size_t)(live ? i : 0) * T1;
  uint8_t* fl = flags + (size_t)(live ? i : 0) * T1;
  PlonkStage1 s;
  FrM acc_inv = {{0, 0, 0, 0}};
  int st_chain = PL_MALFORMED;
  PL_MARK(0);
#if defined(BN254_PLONK_MARKS)
  if (blockIdx.x == 0 && threadIdx.x == 0) g_plonk_sha_n = 0;
#endif
  if (helper) {
    if (live) {
      PL_MARK_H(20);
      {
        // the KZG batching scalar: 384 bits of the call's ChaCha20 stream (blocks 3i .. 3i+2) reduced mod r, as the host path draws it
        uint32_t lw[12];
        for (int j = 0; j < 3; j++) chacha20_block4(lw + 4 * j, lam_key, 3u * i + (uint32_t)j);
        uint8_t lb[48];
        for (int j = 0; j < 12; j++) { lb[4 * j] = (uint8_t)lw[j]; lb[4 * j + 1] = (uint8_t)(lw[j] >> 8); lb[4 * j + 2] = (uint8_t)(lw[j] >> 16); lb[4 * j + 3] = (uint8_t)(lw[j] >> 24); }
        wk.lambda = F.from_be_reduce(lb, 48);
      }
      for (int k = 0; k < T1; k++) { for (int q = 0; q < 18; q++) t[k].pt[q] = 0; for (int q = 0; q < 8; q++) t[k].k[q] = 0; fl[k] = 0; }
      PL_MARK_H(21);
      const int st = parse_plonk_proof(wk.pr, my_proof, stride);                    // lib.rs:70
      PL_MARK_H(22);
      if (st == PL_OK) for (uint32_t k = 0; k < wk.pr.n_bsb; k++) wk.h2f[k] = bsb22_hash_to_field(my_proof + wk.pr.off_bsb + 64 * (size_t)k);
      wk.parse_status = st;
      PL_MARK_H(23);
    }
  } else if (live) {
    PlonkLayout lay;
    if (plonk_proof_layout(lay, my_proof, stride)) {
      st_chain = PlonkStage1::counts(*key, lay.n_bsb, lay.n_claimed, n_public);
      if (st_chain == PL_OK) st_chain = s.chain(*key, my_proof, my_inputs, n_public, wk, lay.off_bsb, lay.n_bsb);
      if (st_chain == PL_OK) acc_inv = F.inverse(s.acc);
    }
    PL_MARK(13);
  }
  __syncthreads();
  if (helper || !live) return;
  PL_MARK(12);
  int st = wk.parse_status;                     // a malformed layout fails the parser too, with that or an earlier point error
  if (st == PL_OK) st = st_chain;
  if (st == PL_OK) st = s.b(acc_inv, t, fl, wk.h2f);
  PL_MARK(11);
  if (st != PL_OK) for (int k = 0; k < T1; k++) { for (int q = 0; q < 18; q++) t[k].pt[q] = 0; for (int q = 0; q < 8; q++) t[k].k[q] = 0; fl[k] = 0; }
  wk.status = st;
}
// k_plonk_stage1 for a batch over many keys (bn254_keys.h): the 64 slots of the workgroup are one granule, so the key and the width of the input rows come from that
// granule's descriptor.  recs / inputs: the pass's records and rows in SLOT order (k_plonk_keys_gather), rec_stride / in_stride bytes apart; proof_len: the caller's
// proof_stride, the length the parser is told; lane_stride: one launch-wide value, from the widest staged key
__global__ void __launch_bounds__(128) k_plonk_stage1_keys(const PlonkKeyDesc* __restrict__ desc, uint32_t n_keys, const uint32_t* __restrict__ granule_key,
                                                           const uint8_t* __restrict__ recs, size_t rec_stride, size_t proof_len, const uint8_t* __restrict__ inputs, size_t in_stride,
                                                           uint32_t n, ChaChaKey lam_key, PlonkWork* work, MsmTerm* terms, uint8_t* flags, int T1, uint32_t lane_stride) {
  const PlonkKeyView kv = plonk_keys_view(desc, granule_key, blockIdx.x * 64u, n_keys);
  const uint8_t* my_inputs;
  const uint8_t* my_proof = pl_stage_lds_rows(recs, rec_stride, inputs, in_stride, (size_t)kv.n_public, n, lane_stride, &my_inputs);
  pl_stage1_body((const PlonkKey*)kv.key, my_proof, my_inputs, proof_len, (size_t)kv.n_public, n, lam_key, work, terms, flags, T1);
}

// one body for k_plonk_stage2 and k_plonk_stage2_keys
__device__ __forceinline__ void pl_stage2_body(const PlonkKey* __restrict__ key, const uint8_t* my_proof, uint32_t n, PlonkWork* __restrict__ work, const uint32_t* __restrict__ lin_words,
                                               const uint8_t* __restrict__ lin_inf, MsmTerm* __restrict__ terms, uint8_t* __restrict__ flags, uint8_t* __restrict__ status, int TT, int T2,
                                               const ChaChaKey& w_key, int weighted) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  MsmTerm* t = terms + (size_t)i * TT;
  uint8_t* fl = flags + (size_t)i * TT;
  for (int k = 0; k < TT; k++) { for (int q = 0; q < 18; q++) t[k].pt[q] = 0; for (int q = 0; q < 8; q++) t[k].k[q] = 0; fl[k] = 0; }
  PlonkWork& wk = work[i];
  PL_MARK(16);
  if (wk.status == PL_OK) {
    wk.pr.raw = my_proof;
    uint32_t lw[16];
    for (int q = 0; q < 16; q++) lw[q] = lin_words[(size_t)i * 16 + q];
    FrM wgt = {{0, 0, 0, 0}};
    if (weighted) {
      // BN254_FLAG_RLC: the proof's weight in the pass's joint pairing check -- 128 bits of the call's second ChaCha20 stream, forced odd (non-zero)
      uint32_t rw[4];
      chacha20_block4(rw, w_key, i);
      uint8_t rb[16];
      rw[0] |= 1u;
      for (int j = 0; j < 4; j++) { rb[15 - 4 * j] = (uint8_t)rw[j]; rb[14 - 4 * j] = (uint8_t)(rw[j] >> 8); rb[13 - 4 * j] = (uint8_t)(rw[j] >> 16); rb[12 - 4 * j] = (uint8_t)(rw[j] >> 24); }
      wgt = fr_ctx().from_be_reduce(rb, 16);
    }
    plonk_stage2(*key, my_proof, wk, lw, lin_inf[i] != 0, t, fl, t + T2, weighted ? &wgt : nullptr);      // ONE copy of the stage in the kernel (two were 22 us of instruction fetch)
    status[i] = BN254_ST_PENDING;
  } else {
    status[i] = (uint8_t)wk.status;
  }
}
__global__ void __launch_bounds__(64) k_plonk_stage2(const PlonkKey* __restrict__ key, const uint8_t* __restrict__ proofs, size_t stride, uint32_t n,
                                                     PlonkWork* __restrict__ work, const uint32_t* __restrict__ lin_words, const uint8_t* __restrict__ lin_inf,
                                                     MsmTerm* __restrict__ terms, uint8_t* __restrict__ flags, uint8_t* __restrict__ status, int TT, int T2, uint32_t lane_stride,
                                                     ChaChaKey w_key, int weighted) {
  const uint8_t* unused_inputs;
  const uint8_t* my_proof = pl_stage_lds(proofs, stride, proofs, 0, n, lane_stride, &unused_inputs);
  pl_stage2_body(key, my_proof, n, work, lin_words, lin_inf, terms, flags, status, TT, T2, w_key, weighted);
}
__global__ void __launch_bounds__(64) k_plonk_stage2_keys(const PlonkKeyDesc* __restrict__ desc, uint32_t n_keys, const uint32_t* __restrict__ granule_key,
                                                          const uint8_t* __restrict__ recs, size_t rec_stride, uint32_t n, PlonkWork* __restrict__ work,
                                                          const uint32_t* __restrict__ lin_words, const uint8_t* __restrict__ lin_inf, MsmTerm* __restrict__ terms, uint8_t* __restrict__ flags,
                                                          uint8_t* __restrict__ status, int TT, int T2, uint32_t lane_stride, ChaChaKey w_key, int weighted) {
  const PlonkKeyView kv = plonk_keys_view(desc, granule_key, blockIdx.x * 64u, n_keys);
  const uint8_t* unused_inputs;
  const uint8_t* my_proof = pl_stage_lds_rows(recs, rec_stride, recs, 0, 0, n, lane_stride, &unused_inputs);
  pl_stage2_body((const PlonkKey*)kv.key, my_proof, n, work, lin_words, lin_inf, terms, flags, status, TT, T2, w_key, weighted);
}

}  // namespace bn254

using namespace bn254;
namespace bn254 { __global__ void k_plonk_dbg_zeta(const PlonkWork* __restrict__ work, uint32_t n, uint8_t* __restrict__ zeta_out, uint8_t* __restrict__ status_out); }
size_t bn254_plonk_work_bytes() { return sizeof(PlonkWork); }
size_t bn254_plonk_key_bytes() { return sizeof(PlonkKey); }
// the field constants of bn254_plonk.hpp (FrCtx, Fp64Ctx: built by host constructors) -> this device's copies; once per device
hipError_t bn254_plonk_dev_init(int device) {
  static std::mutex mu;
  static bool done[64] = {false};
  std::lock_guard<std::mutex> lk(mu);
  if (device < 0 || device >= 64) return hipErrorInvalidDevice;
  if (done[device]) return hipSuccess;
  const FrCtx& F = fr_ctx();
  const Fp64Ctx& C = fp64_ctx();
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_plonk_fr_raw), &F, sizeof(FrCtx));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_plonk_fp64_raw), &C, sizeof(Fp64Ctx));
  if (e == hipSuccess) done[device] = true;
  return e;
}
// The ChaCha20 key and nonce of a pass from its 11 words (null: all zero, for a launch that draws nothing).  weights: the stream of the BN254_FLAG_RLC weights --
// "RLC" in nonce word 2: not the stream the KZG batching scalars come from
static ChaChaKey pl_chacha_key(const uint32_t* words, bool weights) {
  ChaChaKey key;
  for (int i = 0; i < 8; i++) key.k[i] = words ? words[i] : 0u;
  for (int i = 0; i < 3; i++) key.nonce[i] = words ? words[8 + i] : 0u;
  if (weights) key.nonce[2] ^= 0x00524c43u;
  return key;
}
hipError_t bn254_launch_plonk_stage1(const void* d_key, const uint8_t* d_proofs, size_t stride, const uint8_t* d_inputs, size_t n_public, size_t n, const uint32_t lam_key[11],
                                     void* d_work, void* d_terms, uint8_t* d_flags, int T1, hipStream_t s) {
  const ChaChaKey key = pl_chacha_key(lam_key, false);
  const uint32_t ls = pl_lane_stride(stride, n_public);
  const size_t lds = 16 + 64 * (size_t)ls + 64 * (size_t)PL_HELPER_SHA_STRIDE;     // + the SHA blocks of the helper wavefront's lanes (bn254_plonk.hpp::pl_lane_lds)
  if (lds > 65536) { hipError_t ae = hipFuncSetAttribute((const void*)k_plonk_stage1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (ae != hipSuccess) return ae; }
  hipLaunchKernelGGL(k_plonk_stage1, dim3((unsigned)((n + 63) / 64)), dim3(128), lds, s, (const PlonkKey*)d_key, d_proofs, stride, d_inputs, n_public, (uint32_t)n, key,
                     (PlonkWork*)d_work, (MsmTerm*)d_terms, d_flags, T1, ls);
  return hipGetLastError();
}
// the same over the slots of a batch over many keys: recs / inputs in slot order (rec_stride / in_stride apart), the key per granule.  staged_public: the most inputs
// any key of the list stages in LDS (keys above PL_STAGE_MAX_INPUT / 32 read theirs from the rows): it sizes the one lane stride of the launch
hipError_t bn254_launch_plonk_stage1_keys(const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const uint8_t* d_recs, size_t rec_stride, size_t proof_len,
                                          const uint8_t* d_inputs, size_t in_stride, size_t staged_public, size_t n, const uint32_t lam_key[11], void* d_work, void* d_terms,
                                          uint8_t* d_flags, int T1, hipStream_t s) {
  const ChaChaKey key = pl_chacha_key(lam_key, false);
  const uint32_t ls = pl_lane_stride(rec_stride, staged_public);
  const size_t lds = 16 + 64 * (size_t)ls + 64 * (size_t)PL_HELPER_SHA_STRIDE;
  if (lds > 65536) { hipError_t ae = hipFuncSetAttribute((const void*)k_plonk_stage1_keys, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (ae != hipSuccess) return ae; }
  hipLaunchKernelGGL(k_plonk_stage1_keys, dim3((unsigned)((n + 63) / 64)), dim3(128), lds, s, desc, n_keys, granule_key, d_recs, rec_stride, proof_len, d_inputs, in_stride, (uint32_t)n,
                     key, (PlonkWork*)d_work, (MsmTerm*)d_terms, d_flags, T1, ls);
  return hipGetLastError();
}
// weight_key != nullptr: BN254_FLAG_RLC over a list -- every scalar of a slot's two sums carries the slot's weight (the weight stream of the single-key launch)
hipError_t bn254_launch_plonk_stage2_keys(const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const uint8_t* d_recs, size_t rec_stride, size_t n,
                                          void* d_work, const uint32_t* d_lin_words, const uint8_t* d_lin_inf, void* d_terms, uint8_t* d_flags, uint8_t* d_status, int TT, int T2,
                                          const uint32_t* weight_key /* 11 words or nullptr */, hipStream_t s) {
  const ChaChaKey wkey = pl_chacha_key(weight_key, true);
  const uint32_t ls = pl_lane_stride(rec_stride, 0);
  if (16 + 64 * (size_t)ls > 65536) { hipError_t ae = hipFuncSetAttribute((const void*)k_plonk_stage2_keys, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(16 + 64 * (size_t)ls)); if (ae != hipSuccess) return ae; }
  hipLaunchKernelGGL(k_plonk_stage2_keys, dim3((unsigned)((n + 63) / 64)), dim3(64), 16 + 64 * (size_t)ls, s, desc, n_keys, granule_key, d_recs, rec_stride, (uint32_t)n, (PlonkWork*)d_work,
                     d_lin_words, d_lin_inf, (MsmTerm*)d_terms, d_flags, d_status, TT, T2, ls, wkey, weight_key ? 1 : 0);
  return hipGetLastError();
}
// weight_key != nullptr: BN254_FLAG_RLC -- every scalar of the proof's two sums carries the proof's weight (the call's key with another nonce word: a stream of its own)
hipError_t bn254_launch_plonk_stage2(const void* d_key, const uint8_t* d_proofs, size_t stride, size_t n, void* d_work, const uint32_t* d_lin_words, const uint8_t* d_lin_inf,
                                     void* d_terms, uint8_t* d_flags, uint8_t* d_status, int TT, int T2, const uint32_t* weight_key /* 11 words or nullptr */, hipStream_t s) {
  const ChaChaKey wkey = pl_chacha_key(weight_key, true);
  const uint32_t ls = pl_lane_stride(stride, 0);
  if (16 + 64 * (size_t)ls > 65536) { hipError_t ae = hipFuncSetAttribute((const void*)k_plonk_stage2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(16 + 64 * (size_t)ls)); if (ae != hipSuccess) return ae; }
  hipLaunchKernelGGL(k_plonk_stage2, dim3((unsigned)((n + 63) / 64)), dim3(64), 16 + 64 * (size_t)ls, s, (const PlonkKey*)d_key, d_proofs, stride, (uint32_t)n, (PlonkWork*)d_work, d_lin_words,
                     d_lin_inf, (MsmTerm*)d_terms, d_flags, d_status, TT, T2, ls, wkey, weight_key ? 1 : 0);
  return hipGetLastError();
}

// ---- known-answer self-test of the device stages, run once per (key, device) before the key is used there ------------------------------------------------------
// Round 4 met a build in which k_plonk_stage1 derived a wrong first challenge from a correct SHA-256 digest; round 5 rebuilt that flag combination (FrCtx::mul_w32 inlined
// by force, no register barrier in FrCtx::from_be32: tools/gpu_repro.sh) and the defect had MOVED -- the challenges were right, the opening check behind them rejected the
// reference's valid fixtures (the reduced test cases are in tools/repro/, its README.md says how to build and read them).  Two source-level workarounds are
// in; the cause inside the compiler is not known, and a deployment does not run the GPU test suite -- so the library checks THE KERNELS IT SHIPS, on THIS device, against
// the host's compile of the same stage source (which multiplies in the 64-bit form), end to end:
//   * a synthetic proof whose points are the key's own (on the curve), random scalars and the key's number of public inputs, with claimed[0] set to the value the opening
//     check expects (computed by a first host run: PlonkWork::lin_opening) -- so the proof passes every check of stage 1 and the WHOLE stage runs: parser, transcripts,
//     zeta^n, the batched inversion, the public-input sum, BSB22 hash-to-field, the opening check, the scalars of the linearised-polynomial digest and their GLV split;
//   * stage 2 on a fixed digest: the folding transcript, the folded evaluation, lambda, the scalars of the KZG check.
// Compared: both stages' status, zeta, lambda, every hash-to-field value, and every MSM term (point digits, scalar words, flag byte) of both stages, byte for byte.
// A mismatch fails the call that wanted to use the key (BN254_E_HIP with this text): wrong scalars flip verdicts.  Cost: two 1-proof launches, ~2 ms, once per key and device.
hipError_t bn254_plonk_self_test(const void* key_host, const void* d_key, std::string* why) {
  const PlonkKey& key = *(const PlonkKey*)key_host;
  why->clear();
  if (key.nb_public > 4096 || key.n_cci != key.n_qcp) return hipSuccess;          // (a key no proof can satisfy: stage 1 stops at the count checks; nothing to compare)
  const FrCtx& F = fr_ctx();
  const uint32_t q = key.n_qcp;
  const size_t n_pub = (size_t)key.nb_public, len = 516 + 32 * (size_t)(6 + q) + 100 + 64 * (size_t)q;
  std::vector<uint8_t> proof(len), inputs(32 * n_pub + 4);
  uint64_t sm = 0x5e1f7e57b254ull ^ key.size;
  auto next = [&sm] { uint64_t z = (sm += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); };
  for (auto& b : proof) b = (uint8_t)next();
  for (auto& b : inputs) b = (uint8_t)next();
  for (int i = 0; i < 8; i++) memcpy(&proof[64 * (size_t)i], key.enc[i], 64);                       // l r o z h0 h1 h2 batch_h := key points
  proof[512] = 0; proof[513] = 0; proof[514] = 0; proof[515] = (uint8_t)(6 + q);
  const size_t off_zs = 516 + 32 * (size_t)(6 + q);
  memcpy(&proof[off_zs], key.enc[3], 64);
  proof[off_zs + 96] = 0; proof[off_zs + 97] = 0; proof[off_zs + 98] = 0; proof[off_zs + 99] = (uint8_t)q;
  for (uint32_t k = 0; k < q; k++) memcpy(&proof[off_zs + 100 + 64 * (size_t)k], key.enc[(4 + k) % 8], 64);
  uint32_t lam_key[11], lin_words[16];
  for (auto& w : lam_key) w = (uint32_t)next();
  { uint32_t wx[8], wy[8]; fp_to_words(wx, key.ql.x); fp_to_words(wy, key.ql.y); memcpy(lin_words, wx, 32); memcpy(lin_words + 8, wy, 32); }      // the "digest" stage 2 folds: a key point
  const int T1 = plonk_stage1_terms(key), T2 = plonk_stage2_terms(key), TT = T2 + 2;
  // ---- host: the same stage source, compiled for the host.  First run: what must claimed[0] be?  Second run: the proof passes.
  PlonkWork hw; memset((void*)&hw, 0, sizeof hw);
  std::vector<MsmTerm> ht1((size_t)T1), ht2((size_t)TT); std::vector<uint8_t> hf1((size_t)T1), hf2((size_t)TT);
  int hst = PL_MALFORMED;
  for (int pass = 0; pass < 2; pass++) {
    PlonkStage1 hs;
    memset((void*)ht1.data(), 0, ht1.size() * sizeof(MsmTerm)); memset(hf1.data(), 0, hf1.size());
    hst = hs.a(key, proof.data(), len, inputs.data(), n_pub, hw);
    if (hst == PL_OK) hst = hs.b(F.inverse(hs.acc), ht1.data(), hf1.data());
    if (pass == 0) {
      if (hst != PL_OPENING) break;                                                  // (PL_OK already: a 2^-254 event; anything else: compare what there is)
      F.to_be(&proof[516], hw.lin_opening);
    }
  }
  {
    const ChaChaKey ck = pl_chacha_key(lam_key, false);
    uint32_t lw[12]; for (int j = 0; j < 3; j++) chacha20_block4(lw + 4 * j, ck, (uint32_t)j);
    uint8_t lb[48]; for (int j = 0; j < 12; j++) { lb[4 * j] = (uint8_t)lw[j]; lb[4 * j + 1] = (uint8_t)(lw[j] >> 8); lb[4 * j + 2] = (uint8_t)(lw[j] >> 16); lb[4 * j + 3] = (uint8_t)(lw[j] >> 24); }
    hw.lambda = F.from_be_reduce(lb, 48);
  }
  hw.status = hst;
  if (hst == PL_OK) { hw.pr.raw = proof.data(); plonk_stage2(key, proof.data(), hw, lin_words, false, ht2.data(), hf2.data(), ht2.data() + T2); }
  // ---- device: the shipped kernels, one proof
  uint8_t* dbuf = nullptr;
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t o_in = up16(len), o_work = up16(o_in + inputs.size()), o_t1 = up16(o_work + sizeof(PlonkWork)), o_f1 = o_t1 + (size_t)T1 * sizeof(MsmTerm), o_t2 = up16(o_f1 + (size_t)T1),
               o_f2 = o_t2 + (size_t)TT * sizeof(MsmTerm), o_lin = up16(o_f2 + (size_t)TT), o_inf = o_lin + 64, o_st = o_inf + 16, total = o_st + 16;
  hipError_t e = hipMalloc((void**)&dbuf, total);
  if (e != hipSuccess) return e;
  PlonkWork dw; memset((void*)&dw, 0, sizeof dw);
  std::vector<MsmTerm> dt1((size_t)T1), dt2((size_t)TT); std::vector<uint8_t> df1((size_t)T1), df2((size_t)TT);
  uint8_t dst2 = 0xEE;
  e = hipMemset(dbuf, 0, total);
  if (e == hipSuccess) e = hipMemcpy(dbuf, proof.data(), len, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dbuf + o_in, inputs.data(), inputs.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dbuf + o_lin, lin_words, 64, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = bn254_launch_plonk_stage1(d_key, dbuf, len, dbuf + o_in, n_pub, 1, lam_key, dbuf + o_work, dbuf + o_t1, dbuf + o_f1, T1, nullptr);
  if (e == hipSuccess) e = bn254_launch_plonk_stage2(d_key, dbuf, len, 1, dbuf + o_work, (const uint32_t*)(dbuf + o_lin), dbuf + o_inf, dbuf + o_t2, dbuf + o_f2, dbuf + o_st, TT, T2, nullptr, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy((void*)&dw, dbuf + o_work, sizeof(PlonkWork), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy((void*)dt1.data(), dbuf + o_t1, dt1.size() * sizeof(MsmTerm), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(df1.data(), dbuf + o_f1, df1.size(), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy((void*)dt2.data(), dbuf + o_t2, dt2.size() * sizeof(MsmTerm), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(df2.data(), dbuf + o_f2, df2.size(), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&dst2, dbuf + o_st, 1, hipMemcpyDeviceToHost);
  (void)hipFree(dbuf);
  if (e != hipSuccess) return e;
  auto hex = [&F](const FrM& v) { uint8_t b[32]; F.to_be(b, v); char t[65]; for (int i = 0; i < 32; i++) snprintf(t + 2 * i, 3, "%02x", b[i]); return std::string(t, 16) + ".."; };
  auto first_diff = [](const std::vector<MsmTerm>& a, const std::vector<MsmTerm>& b, const std::vector<uint8_t>& fa, const std::vector<uint8_t>& fb) {
    for (size_t k = 0; k < a.size(); k++) if (memcmp(&a[k], &b[k], sizeof(MsmTerm)) != 0 || fa[k] != fb[k]) return (int)k;
    return -1;
  };
  if (!F.eq(dw.zeta, hw.zeta)) *why = "zeta (the chained Fiat-Shamir challenges): device " + hex(dw.zeta) + " host " + hex(hw.zeta);
  else if (!F.eq(dw.lambda, hw.lambda)) *why = "lambda (ChaCha20 bytes reduced mod r): device " + hex(dw.lambda) + " host " + hex(hw.lambda);
  else if (dw.status != hst) *why = "stage-1 status: device " + std::to_string(dw.status) + " host " + std::to_string(hst) + (F.eq(dw.lin_opening, hw.lin_opening) ? "" : "; the linearised polynomial's opening: device " + hex(dw.lin_opening) + " host " + hex(hw.lin_opening));
  else for (uint32_t k = 0; k < q && why->empty(); k++) {
    const FrM hh = bsb22_hash_to_field(&proof[off_zs + 100 + 64 * (size_t)k]);
    if (!F.eq(dw.h2f[k], hh)) *why = "BSB22 hash-to-field " + std::to_string(k) + ": device " + hex(dw.h2f[k]) + " host " + hex(hh);
  }
  if (why->empty() && hst == PL_OK) {
    const int d1 = first_diff(dt1, ht1, df1, hf1);
    if (d1 >= 0) *why = "term " + std::to_string(d1) + " of the linearised-polynomial digest (stage 1 scalars / GLV split)";
    else if (dst2 != BN254_ST_PENDING) *why = "stage-2 status byte " + std::to_string((int)dst2);
    else { const int d2 = first_diff(dt2, ht2, df2, hf2); if (d2 >= 0) *why = "term " + std::to_string(d2) + " of the KZG check (stage 2: folding transcript, folded evaluation, lambda)"; }
  }
  if (!why->empty()) *why = "PlonK device self-test failed (the stage kernels on this GPU disagree with the host's compile of the same source) -- " + *why;
  return hipSuccess;
}

namespace bn254 {
// probe for the parity tests: zeta (the last of the four chained Fiat-Shamir challenges: it depends on gamma, beta and alpha) and the stage-1 status
// of every proof as the DEVICE computed them -- canonical 32-byte big-endian values
__global__ void k_plonk_dbg_zeta(const PlonkWork* __restrict__ work, uint32_t n, uint8_t* __restrict__ zeta_out, uint8_t* __restrict__ status_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  uint8_t z[32];
  fr_ctx().to_be(z, work[i].zeta);
  for (int j = 0; j < 32; j++) zeta_out[(size_t)i * 32 + j] = work[i].status == PL_OK || work[i].status == PL_OPENING ? z[j] : 0;
  status_out[i] = (uint8_t)work[i].status;
}
// probe for the value tests (bn254_dbg_plonk_stages): what both stages and the digest MSM left for proof (slot) i, 432 bytes, field values canonical big-endian:
//   0 stage-1 status | 1 the status byte after stage 2 as stored | 2 the digest is the identity | 3 .. 15 zero
//   16 zeta | 48 lambda | 80 lin_opening | 112 the linearised-polynomial digest (x | y, zero for the identity) | 176 h2f[0 .. n_h2f)
// Everything but the two status bytes is zero for a proof stage 1 decided, except zeta on an opening mismatch (as k_plonk_dbg_zeta)
__global__ void __launch_bounds__(64) k_plonk_dbg_stages(const PlonkWork* __restrict__ work, const uint32_t* __restrict__ lin_words, const uint8_t* __restrict__ lin_inf,
                                                         const uint8_t* __restrict__ status, uint32_t n, uint32_t n_h2f, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const FrCtx& F = fr_ctx();
  const PlonkWork& wk = work[i];
  uint8_t* o = out + (size_t)i * 432;
  for (int j = 0; j < 432; j++) o[j] = 0;
  o[0] = (uint8_t)wk.status; o[1] = status[i];
  uint8_t b[32];
  auto put = [&](int at, const FrM& v) { F.to_be(b, v); for (int j = 0; j < 32; j++) o[at + j] = b[j]; };
  if (wk.status == PL_OK || wk.status == PL_OPENING) put(16, wk.zeta);
  if (wk.status != PL_OK) return;
  put(48, wk.lambda); put(80, wk.lin_opening);
  if (lin_inf[i]) o[2] = 1;
  else {
    uint32_t w[16];
    for (int q = 0; q < 16; q++) w[q] = lin_words[(size_t)i * 16 + q];
    words_to_be(b, w); for (int j = 0; j < 32; j++) o[112 + j] = b[j];
    words_to_be(b, w + 8); for (int j = 0; j < 32; j++) o[144 + j] = b[j];
  }
  for (uint32_t k = 0; k < n_h2f && k < (uint32_t)PLONK_MAX_QCP; k++) put(176 + 32 * (int)k, wk.h2f[k]);
}
}  // namespace bn254
#if defined(BN254_PLONK_MARKS)
// diagnostics build: the clock stamps of the last stage launches (100 MHz ticks; bn254_plonk.hpp::PL_MARK)
extern "C" int bn254_dbg_plonk_marks(unsigned long long out[32]) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plonk_marks), 32 * sizeof(unsigned long long)); }
// ... and the dumped intermediate values of the first lane (64 x 32 bytes, little-endian limbs; bn254_plonk.hpp::PL_DUMP)
extern "C" int bn254_dbg_plonk_sha_dump_device(uint32_t out[32 * 24], uint32_t* n) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plonk_sha_dump), 32 * 24 * 4);
  if (e == hipSuccess) e = hipMemcpyFromSymbol(n, HIP_SYMBOL(g_plonk_sha_n), 4);
  return (int)e;
}
extern "C" int bn254_dbg_plonk_dump_device(uint8_t out[64 * 32]) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_plonk_dump), 64 * 32); }
#endif
hipError_t bn254_launch_plonk_dbg_zeta(const void* d_work, size_t n, uint8_t* d_zeta, uint8_t* d_status, hipStream_t s) {
  hipLaunchKernelGGL(k_plonk_dbg_zeta, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const PlonkWork*)d_work, (uint32_t)n, d_zeta, d_status);
  return hipGetLastError();
}
hipError_t bn254_launch_plonk_dbg_stages(const void* d_work, const uint32_t* d_lin_words, const uint8_t* d_lin_inf, const uint8_t* d_status, size_t n, uint32_t n_h2f, uint8_t* d_out,
                                         hipStream_t s) {
  if (n_h2f > (uint32_t)PLONK_MAX_QCP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_plonk_dbg_stages, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const PlonkWork*)d_work, d_lin_words, d_lin_inf, d_status, (uint32_t)n, n_h2f, d_out);
  return hipGetLastError();
}
