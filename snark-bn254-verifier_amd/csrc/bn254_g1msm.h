// bn254_g1msm.h -- batch G1 multi-scalar multiplication over caller records (include/bn254_verify.h, bn254_g1_msm_batch): what the kernels of bn254_k_g1msm.hip, the host
// code of bn254_capi_g1msm.hip and the host compile behind bn254_dbg_g1_msm_batch(device = -1) share.
//   item i (G1MSM_ITEM_LEN(v, u, s) bytes): v pairs (point x | y, scalar), then u bare points, then s scalars for the call's shared bases -- 32-byte big-endian fields
//   result:  S_i = sum k_t P_t + sum U_t + sum c_j B_j  as 64 bytes x | y (zero: the identity, or an item the loader decided) and a status byte
// The loader (g1msm_load_item, one item per lane) checks the record in the definition's order, reduces the scalars, splits those of the variable terms (glv_decompose)
// and writes the TERM records the rows of bn254_msm.h walk: terms 0 .. v-1 variable, v .. v+u-1 unit, v+u .. v+u+s-1 fixed (the eight canonical scalar words that
// scalar_digit reads; window table j of the handle).  k_g1_msm_rows and k_g1_sum_affine (words form) do the walk; g1msm_store_item turns the sum into bytes.
#pragma once
#include "bn254_kzg.h"

namespace bn254 {

#define G1MSM_MAX_VAR 16
#define G1MSM_MAX_UNIT 4
#define G1MSM_MAX_SHARED 16
#define G1MSM_ITEM_LEN(v, u, s) ((size_t)96 * (size_t)(v) + (size_t)64 * (size_t)(u) + (size_t)32 * (size_t)(s))
static_assert(G1MSM_MAX_VAR <= MSM_MAX_FIXED && G1MSM_MAX_SHARED <= MSM_MAX_FIXED && G1MSM_MAX_UNIT == 4, "the limits are the planner's (bn254_msm.h)");
// items of a pass: at most 2^18, and fewer where the walk's buffers of that many items would pass G1MSM_PASS_BUDGET bytes.  Per item: a term record and its flag byte
// per term (105 bytes), up to MSM_MAX_ROWS rows of 108 bytes, G1_GLV_TAB_BYTES_PER_LANE of window-table scratch per variable term (a large launch walks a term in one
// row), and the sum's sixteen words, its identity flag and the loader's status byte (66 bytes)
#define G1MSM_MAX_PASS ((size_t)1 << 18)
#define G1MSM_PASS_BUDGET ((size_t)1 << 31)
#define G1MSM_BYTES_PER_ITEM(v, u, s) ((size_t)105 * ((size_t)(v) + (size_t)(u) + (size_t)(s)) + (size_t)G1_GLV_TAB_BYTES_PER_LANE * (size_t)(v) + (size_t)108 * MSM_MAX_ROWS + 66)
inline size_t g1msm_max_pass(size_t v, size_t u, size_t s) {
  const size_t m = (G1MSM_PASS_BUDGET / G1MSM_BYTES_PER_ITEM(v, u, s)) & ~(size_t)63;
  return m < G1MSM_MAX_PASS ? m : G1MSM_MAX_PASS;
}
inline bool g1msm_shape_ok(size_t v, size_t u, size_t s) { return v <= G1MSM_MAX_VAR && u <= G1MSM_MAX_UNIT && s <= G1MSM_MAX_SHARED && v + u + s > 0; }
inline MsmShape g1msm_shape(int v, int u, int s) {
  MsmShape sh;
  std::memset(&sh, 0, sizeof sh);
  sh.n_sums = 1; sh.n_var[0] = v; sh.n_unit[0] = u; sh.n_fixed[0] = s;
  for (int t = 0; t < v; t++) sh.var_term[0][t] = (int8_t)t;
  for (int t = 0; t < u; t++) sh.unit_term[0][t] = (int8_t)(v + t);
  for (int t = 0; t < s; t++) { sh.fixed_term[0][t] = (int8_t)(v + u + t); sh.fixed_tab[0][t] = (int8_t)t; }
  return sh;
}

// a scalar of a record, used modulo r: x 2^256 mod r (exact for any x < 2^256), then out of the Montgomery form (kzg_load_opening's rule)
BN_HD Fr8 g1msm_scalar(const uint8_t* p, bool aligned) {
  Fr8 k, r2, one = fr8_zero();
  pb_field_words(k.w, p, aligned);
#pragma unroll
  for (int i = 0; i < 8; i++) r2.w[i] = bn_r2_word(i);
  one.w[0] = 1;
  return fr8_mont_mul(fr8_mont_mul(k, r2), one);
}
BN_HD G1Aff g1msm_point(const uint8_t* p, bool aligned, bool& memb, bool& zero) {
  G1Aff P;
  P.x = pb_field(p, aligned, memb, zero); P.y = pb_field(p + 32, aligned, memb, zero);
  return P;
}
// ---- the loader of one item --------------------------------------------------------------------------------------------------------------------------------------
// rec: the item; nv, nu, ns: the call's shape (uniform over a launch); dead_bases: bit j set when shared base j is the identity (its scalar is written as zero, so its
// table is never consulted); strict: BN254_FLAG_STRICT_SCALARS.  terms / flags: the item's nv + nu + ns records.  Returns the decided error or BN254_ST_PENDING.  The
// order is the definition's: strict scalars, then the points in record order (a coordinate >= p before the curve equation).
BN_HD int g1msm_load_item(const uint8_t* rec, bool aligned, int nv, int nu, int ns, uint32_t dead_bases, bool strict, int32_t* terms, uint8_t* flags) {
  const int n_terms = nv + nu + ns;
  const uint8_t* units = rec + 96 * (size_t)nv;
  const uint8_t* shared = units + 64 * (size_t)nu;
  int err = 0;
  if (strict) {
    bool big = false;
#pragma unroll 1
    for (int t = 0; t < nv + ns; t++) {
      uint32_t kw[8];
      pb_field_words(kw, t < nv ? rec + 96 * (size_t)t + 64 : shared + 32 * (size_t)(t - nv), aligned);
      big |= words_ge(kw, BN_R_WORDS);
    }
    if (big) err = BN254_ST_NOT_MEMBER;
  }
#pragma unroll 1
  for (int t = 0; t < nv + nu; t++) {
    bool memb = true, zero = true;
    const G1Aff P = g1msm_point(t < nv ? rec + 96 * (size_t)t : units + 64 * (size_t)(t - nv), aligned, memb, zero);
    if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!zero && !g1_on_curve(P)) err = BN254_ST_NOT_ON_CURVE; }
  }
  if (err) {
    // a decided item: records the walk reads without meaning (every term dead, every scalar zero)
    for (int t = 0; t < n_terms; t++) { for (int q = 0; q < MSM_TERM_DWORDS; q++) terms[t * MSM_TERM_DWORDS + q] = 0; flags[t] = 1; }
    return err;
  }
  // the points are read again from the record: no array of them stays live
#pragma unroll 1
  for (int t = 0; t < nv; t++) {
    bool memb = true, zero = true;
    const G1Aff P = g1msm_point(rec + 96 * (size_t)t, aligned, memb, zero);
    kzg_put_var(terms + (size_t)t * MSM_TERM_DWORDS, flags + t, P, g1msm_scalar(rec + 96 * (size_t)t + 64, aligned), zero);
  }
#pragma unroll 1
  for (int t = 0; t < nu; t++) {
    bool memb = true, zero = true;
    const G1Aff P = g1msm_point(units + 64 * (size_t)t, aligned, memb, zero);
    kzg_put_unit(terms + (size_t)(nv + t) * MSM_TERM_DWORDS, flags + nv + t, P, zero);
  }
#pragma unroll 1
  for (int j = 0; j < ns; j++) {
    const Fr8 c = g1msm_scalar(shared + 32 * (size_t)j, aligned);
    const bool dead = ((dead_bases >> j) & 1u) != 0;
    int32_t* t = terms + (size_t)(nv + nu + j) * MSM_TERM_DWORDS;
#pragma unroll
    for (int q = 0; q < 18; q++) t[q] = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) t[18 + q] = dead ? 0 : (int32_t)c.w[q];
    flags[nv + nu + j] = (uint8_t)(dead ? 1 : 0);
  }
  return BN254_ST_PENDING;
}
// ---- the store of one item ---------------------------------------------------------------------------------------------------------------------------------------
// st: the loader's status byte; words: the sum as k_g1_sum_affine left it (x | y, sixteen little-endian words, canonical); inf: its identity flag.  out: 64 bytes
// x | y big-endian, zero for the identity and for a decided item; *status: BN254_ST_ACCEPT or the loader's error.  aligned: out is 4-byte aligned (dword stores)
BN_HD void g1msm_store_item(uint8_t* out, uint8_t* status, int st, const uint32_t* words, bool inf, bool aligned) {
  const bool pend = (st & BN254_ST_PENDING) != 0, zero = !pend || inf;
  if (aligned) {
    uint32_t* o = (uint32_t*)out;
#pragma unroll
    for (int k = 0; k < 8; k++) { o[k] = zero ? 0u : __builtin_bswap32(words[7 - k]); o[8 + k] = zero ? 0u : __builtin_bswap32(words[15 - k]); }
  } else {
    uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    words_to_be(out, zero ? z : words); words_to_be(out + 32, zero ? z : words + 8);
  }
  *status = (uint8_t)(pend ? BN254_ST_ACCEPT : st);
}

// ---- launches (bn254_k_g1msm.hip) --------------------------------------------------------------------------------------------------------------------------------
struct G1MsmLoadArgs {
  const uint8_t* items; size_t stride; size_t n;      // device memory, n <= G1MSM_MAX_PASS, stride >= G1MSM_ITEM_LEN(n_var, n_unit, n_shared)
  int n_var, n_unit, n_shared;
  uint32_t dead_bases;
  bool strict;
  uint8_t* status;               // n bytes: the loader's status (BN254_ST_PENDING or the decided error)
  int32_t* terms; uint8_t* flags;                     // n x (n_var + n_unit + n_shared) records
};

}  // namespace bn254

hipError_t bn254_launch_g1msm_load(const bn254::G1MsmLoadArgs& a, hipStream_t s);
// words / inf: what bn254_launch_g1_sum_rows left in its out_words / out_inf form; st: the loader's status bytes; out (64 n bytes) and status (n bytes): the caller's
hipError_t bn254_launch_g1msm_store(const uint32_t* words, const uint8_t* inf, const uint8_t* st, size_t n, uint8_t* out, uint8_t* status, hipStream_t s);
