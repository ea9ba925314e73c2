// bn254_g16_loader.h -- the parse of a raw 256-byte Groth16 record, shared by every kernel that reads one (k_g16_classify, k_g16_prepare: bn254_k_g16_load.hip;
// k_g16_prepare_keys: bn254_k_keys.hip): the staging of a wavefront's 64 records into its LDS rows and the range / on-curve checks of A, B and C, so that a proof the
// one kernel calls decided is decided the same way by the others.
#pragma once
#include "bn254_devws.h"

namespace bn254 {

#define PREP_LDS_ROW 65  // 64 proof dwords + 1 pad: lane-per-proof reads hit 64 different banks
// The records of the 64 lanes of a wavefront -> its LDS rows: lane j holds the index `rec` of ITS record (>= n: none, the row reads as zeros), the wavefront loads record
// readlane(rec, j) as one 256-byte contiguous segment per load instruction.  One routine for the records in batch order (rec = the lane's own index) and for the
// gather of a launch that compacts (rec = slot_proof of the lane's slot).
__device__ __forceinline__ void g16_stage_records(uint32_t* wl, const uint8_t* __restrict__ proofs, size_t stride, uint32_t n, int lane, uint32_t rec_of_lane) {
  const bool aligned = ((((uintptr_t)proofs) | stride) & 3) == 0;
  if (aligned) {
    // SIXTEEN records per step, so that sixteen loads are in flight together (one record at a time compiled to load / wait / store: 64 dependent round trips to HBM
    // per wavefront)
    for (int j0 = 0; j0 < 64; j0 += 16) {
      uint32_t v[16];
#pragma unroll
      for (int u = 0; u < 16; u++) { const uint32_t rec = (uint32_t)__builtin_amdgcn_readlane((int)rec_of_lane, j0 + u); v[u] = rec < n ? *(const uint32_t*)(proofs + (size_t)rec * stride + (size_t)lane * 4) : 0u; }
#pragma unroll
      for (int u = 0; u < 16; u++) wl[(j0 + u) * PREP_LDS_ROW + lane] = v[u];
    }
  } else {
    for (int j = 0; j < 64; j++) {
      const uint32_t rec = (uint32_t)__builtin_amdgcn_readlane((int)rec_of_lane, j);
      uint32_t v = 0;
      if (rec < n) {
        const uint8_t* p = proofs + (size_t)rec * stride + (size_t)lane * 4;
        v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
      }
      wl[j * PREP_LDS_ROW + lane] = v;
    }
  }
}
// The loader's checks of A and of B from a lane's LDS row (my: the record's 64 dwords): the first error in the reference's order, A, then B (member, curve); 0: none.
// k_g16_prepare, k_g16_prepare_keys and k_g16_classify all decide through these two, so a proof the one calls decided is decided the same way by the others.
__device__ __forceinline__ int g16_parse_a(const uint32_t* my, G1Aff& A) {
  uint32_t d[8], wx[8], wy[8];
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[k];
  be_field_to_words(wx, d);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[8 + k];
  be_field_to_words(wy, d);
  const bool memb = words_lt_p(wx) & words_lt_p(wy);
  A.x = fp_from_words(wx); A.y = fp_from_words(wy);
  return !memb ? BN254_ST_NOT_MEMBER : !g1_on_curve(A) ? BN254_ST_NOT_ON_CURVE : 0;
}
__device__ __forceinline__ int g16_parse_b(const uint32_t* my, G2Aff& B, int err) {   // B : x.c1 | x.c0 | y.c1 | y.c0
  uint32_t d[8], wx[8];
  bool membb = true;
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[16 + k];
  be_field_to_words(wx, d); membb &= words_lt_p(wx); B.x.c1 = fp_from_words(wx);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[24 + k];
  be_field_to_words(wx, d); membb &= words_lt_p(wx); B.x.c0 = fp_from_words(wx);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[32 + k];
  be_field_to_words(wx, d); membb &= words_lt_p(wx); B.y.c1 = fp_from_words(wx);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[40 + k];
  be_field_to_words(wx, d); membb &= words_lt_p(wx); B.y.c0 = fp_from_words(wx);
  if (err == 0) { if (!membb) err = BN254_ST_NOT_MEMBER; else if (!g2_on_curve(B)) err = BN254_ST_NOT_ON_CURVE; }
  return err;
}
// ... and of C: its error is DEFERRED by the kernels that prepare (the r-torsion test of B, the tail of the Miller loop, ranks ahead of it); 0: none
__device__ __forceinline__ int g16_parse_c(const uint32_t* my, G1Aff& C) {
  uint32_t d[8], wx[8], wy[8];
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[48 + k];
  be_field_to_words(wx, d);
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = my[56 + k];
  be_field_to_words(wy, d);
  const bool memb = words_lt_p(wx) & words_lt_p(wy);
  C.x = fp_from_words(wx); C.y = fp_from_words(wy);
  return !memb ? BN254_ST_NOT_MEMBER : !g1_on_curve(C) ? BN254_ST_NOT_ON_CURVE : 0;
}

}  // namespace bn254
