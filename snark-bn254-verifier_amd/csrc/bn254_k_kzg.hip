// bn254_k_kzg.hip -- batch verification of KZG openings (include/bn254_verify.h, bn254_kzg_verify_batch; bn254_kzg.h): the kernels in front of and behind the G1
// walk, one opening (or one group) per lane.
//   k_kzg_load    the opening's record -> status byte and the TERM records k_g1_msm_rows walks (bn254_kzg.h::kzg_load_opening: range and curve checks in record
//                 order, z and y modulo r, under BN254_FLAG_RLC the opening's weight folded into the scalars, glv_decompose); exact form: -H to vp_p(1)
//   k_kzg_fold_load   the loader of a batch-opening record (bn254_kzg_verify_folded_batch; bn254_kzg.h::kzg_fold_load_record): the checks, the transcript hashed straight
//                 from the record, the powers of gamma, KZG_FOLD_TERMS(k, weighted) term records; everything behind it is what follows k_kzg_load
//   k_kzg_ident   behind k_g1_sum_affine (and behind k_plonk_group_sums for the groups of the weighted path): the key's G2 points and the identity bits of a pending
//                 item into the workspace in the pairing batch's layout, the status byte back to BN254_ST_PENDING alone
//   k_kzg_fetch   the probe (bn254_dbg_kzg_fold): the two G1 points of every item as bytes
// The walk itself is bn254_k_msm.hip (k_g1_msm_rows, k_g1_sum_affine into vp_p(0) / vp_p(1)), the group sums k_plonk_group_sums / k_plonk_group_scatter, the check
// bn254_launch_pairing_batch with the load step skipped (mask 0b11, the key's two prepared records).
#include <hip/hip_runtime.h>
#include "bn254_devws.h"
#include "bn254_kzg.h"

namespace bn254 {

// A malformed key (the magic word, the layout version, the header of either record) ends every opening MALFORMED before anything else of the key is read: the rule
// of k_pairing_load_shared.
__global__ void __launch_bounds__(256, 2) k_kzg_load(const int32_t* __restrict__ key, const uint8_t* __restrict__ openings, size_t stride, uint32_t n, int32_t* ws,
                                                     uint8_t* __restrict__ status, int32_t* __restrict__ terms, uint8_t* __restrict__ flags, int strict, int weighted,
                                                     const uint32_t* __restrict__ weights, ChaChaKey wkey) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int n_terms = __builtin_amdgcn_readfirstlane(weighted) ? KZG_TERMS_RLC : KZG_TERMS_EXACT;
  int32_t* t = terms + (size_t)i * (size_t)n_terms * MSM_TERM_DWORDS;
  uint8_t* fl = flags + (size_t)i * (size_t)n_terms;
  const int32_t* k = uni_ptr(key);
  if (!kzg_key_header_ok(k)) {
    for (int q = 0; q < n_terms * MSM_TERM_DWORDS; q++) t[q] = 0;
    for (int q = 0; q < n_terms; q++) fl[q] = 1;
    status[i] = BN254_ST_MALFORMED;
    return;
  }
  DevWs w(ws, n, i);
  const bool aligned = ((((uintptr_t)openings) | stride) & 3) == 0;
  uint32_t wgt[4];
  if (weighted) {
    if (weights) { for (int q = 0; q < 4; q++) wgt[q] = weights[(size_t)i * 4 + q]; wgt[0] |= 1u; }
    else kzg_weight(wgt, wkey, i);
  }
  status[i] = (uint8_t)kzg_load_opening(w, openings + (size_t)i * stride, aligned, k, strict != 0, weighted ? wgt : nullptr, t, fl);
}

// k and data_len are the call's: uniform over the launch, held in scalar registers (the loops over the digests and the blocks of the transcript run in step)
__global__ void __launch_bounds__(256, 2) k_kzg_fold_load(const int32_t* __restrict__ key, const uint8_t* __restrict__ records, size_t stride, uint32_t n, int n_digests, int data_len,
                                                          int32_t* ws, uint8_t* __restrict__ status, int32_t* __restrict__ terms, uint8_t* __restrict__ flags, int strict, int weighted,
                                                          const uint32_t* __restrict__ weights, ChaChaKey wkey, uint8_t* __restrict__ dbg) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int kd = __builtin_amdgcn_readfirstlane(n_digests), dl = __builtin_amdgcn_readfirstlane(data_len);
  const int n_terms = KZG_FOLD_TERMS(kd, __builtin_amdgcn_readfirstlane(weighted) != 0);
  int32_t* t = terms + (size_t)i * (size_t)n_terms * MSM_TERM_DWORDS;
  uint8_t* fl = flags + (size_t)i * (size_t)n_terms;
  uint8_t* dg = dbg ? dbg + 64 * (size_t)i : nullptr;
  const int32_t* k = uni_ptr(key);
  if (!kzg_key_header_ok(k)) {
    for (int q = 0; q < n_terms * MSM_TERM_DWORDS; q++) t[q] = 0;
    for (int q = 0; q < n_terms; q++) fl[q] = 1;
    if (dg) for (int q = 0; q < 64; q++) dg[q] = 0;
    status[i] = BN254_ST_MALFORMED;
    return;
  }
  DevWs w(ws, n, i);
  const bool aligned = ((((uintptr_t)records) | stride) & 3) == 0;
  uint32_t wgt[4];
  if (weighted) {
    if (weights) { for (int q = 0; q < 4; q++) wgt[q] = weights[(size_t)i * 4 + q]; wgt[0] |= 1u; }
    else kzg_weight(wgt, wkey, i);
  }
  status[i] = (uint8_t)kzg_fold_load_record(w, records + (size_t)i * stride, aligned, kd, dl, k, strict != 0, weighted ? wgt : nullptr, t, fl, dg);
}

__global__ void __launch_bounds__(256, 2) k_kzg_ident(const int32_t* __restrict__ key, int32_t* ws, uint8_t* __restrict__ status, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = status[i];
  if (!(st & BN254_ST_PENDING)) return;
  DevWs w(ws, n, i);
  kzg_finish_item(w, uni_ptr(key), st);
  status[i] = BN254_ST_PENDING;
}

__global__ void __launch_bounds__(256, 2) k_kzg_fetch(const int32_t* ws, const uint8_t* __restrict__ status, uint32_t n, uint8_t* __restrict__ out_f, uint8_t* __restrict__ out_h,
                                                      uint8_t* __restrict__ out_inf) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  DevWs w((int32_t*)ws, n, i);
  const bool pend = (status[i] & BN254_ST_PENDING) != 0;
  const uint32_t ident = pend ? pb_ident(w) : 0u;
  for (int j = 0; j < 2; j++) {
    uint8_t* o = (j ? out_h : out_f) + 64 * (size_t)i;
    const bool inf = ((ident >> (2 * j)) & 1u) != 0;
    out_inf[2 * (size_t)i + j] = inf ? 1 : 0;
    if (!pend || inf) { for (int q = 0; q < 64; q++) o[q] = 0; continue; }
    uint32_t v[8];
    fp_to_words(v, w.ld(vp_p(j))); words_to_be(o, v);
    fp_to_words(v, w.ld(vp_p(j) + 1)); words_to_be(o + 32, v);
  }
}

}  // namespace bn254

using namespace bn254;
hipError_t bn254_launch_kzg_load(const KzgLoadArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  if (a.n_digests) {
    if (a.n_digests < 1 || a.n_digests > KZG_FOLD_MAX_DIGESTS || a.data_len < 0 || a.data_len > KZG_FOLD_MAX_DATA || a.n > kzg_fold_max_launch((size_t)a.n_digests) || !a.key ||
        ((uintptr_t)a.key & 3) || !a.openings || a.stride < KZG_FOLD_LEN(a.n_digests, a.data_len) || !a.ws || !a.status || ((uintptr_t)a.status & 3) || !a.terms || !a.flags)
      return hipErrorInvalidValue;
    if (a.n_digests == 1 && !a.dbg) {      // an opening (bn254_kzg.h, KzgLoadArgs): the same kernel, the same time
      hipLaunchKernelGGL(k_kzg_load, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.key, a.openings, a.stride, (uint32_t)a.n, a.ws, a.status, a.terms, a.flags, a.strict ? 1 : 0,
                         a.weighted ? 1 : 0, a.weighted ? a.weights : nullptr, a.wkey);
      return hipGetLastError();
    }
    hipLaunchKernelGGL(k_kzg_fold_load, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.key, a.openings, a.stride, (uint32_t)a.n, a.n_digests, a.data_len, a.ws, a.status, a.terms,
                       a.flags, a.strict ? 1 : 0, a.weighted ? 1 : 0, a.weighted ? a.weights : nullptr, a.wkey, a.dbg);
    return hipGetLastError();
  }
  if (a.n > KZG_MAX_LAUNCH || !a.key || ((uintptr_t)a.key & 3) || !a.openings || a.stride < KZG_OPENING_LEN || !a.ws || !a.status || ((uintptr_t)a.status & 3) || !a.terms || !a.flags)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_kzg_load, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.key, a.openings, a.stride, (uint32_t)a.n, a.ws, a.status, a.terms, a.flags, a.strict ? 1 : 0,
                     a.weighted ? 1 : 0, a.weighted ? a.weights : nullptr, a.wkey);
  return hipGetLastError();
}
hipError_t bn254_launch_kzg_ident(const int32_t* key, int32_t* ws, uint8_t* status, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > (size_t)G16_MAX_LAUNCH || !key || !ws || !status) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_kzg_ident, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, key, ws, status, (uint32_t)n);
  return hipGetLastError();
}
hipError_t bn254_launch_kzg_fetch(const int32_t* ws, const uint8_t* status, size_t n, uint8_t* out_f, uint8_t* out_h, uint8_t* out_inf, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > (size_t)G16_MAX_LAUNCH || !ws || !status || !out_f || !out_h || !out_inf) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_kzg_fetch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws, status, (uint32_t)n, out_f, out_h, out_inf);
  return hipGetLastError();
}
