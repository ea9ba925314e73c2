// bn254_kzg.h -- batch verification of KZG openings (include/bn254_verify.h, bn254_kzg_verify_batch; the reference's plonk/kzg.rs::batch_verify_multi_points, 128-190,
// for openings a caller holds): what the kernels of bn254_k_kzg.hip, the host code of bn254_capi_kzg.hip and the host compile behind bn254_dbg_kzg_fold(device = -1) share.
//   opening i (BN254_KZG_OPENING_LEN bytes): commitment C x | y, quotient H x | y, point z, claimed value y -- 32-byte big-endian each
//   key (BN254_KZG_KEY_LEN bytes, plain data like a prepared G2 record): header | g1 as workspace digits | the prepared records of g2 and tau_g2
//   verdict:   e(C - y g1 + z H, g2) e(-H, tau_g2) == 1,   i.e. the two-pair item (F_i, -H_i) of bn254_pairing_check_batch_shared with both positions shared
// The G1 fold F_i = C_i - y_i g1 + z_i H_i runs on the device: the loader (kzg_load_opening, one opening per lane) checks the record, reduces the scalars, splits them
// (glv_decompose) and writes the TERM records the rows of bn254_msm.h walk; k_g1_sum_affine leaves F_i at vp_p(0) of the pairing workspace.  Under BN254_FLAG_RLC every
// opening carries a fresh odd 128-bit weight r_i folded into its scalars -- F'_i = r_i C_i + (r_i z_i) H_i - (r_i y_i) g1 and H'_i = -r_i H_i -- the weighted points
// of the 64 openings of a wavefront are summed and ONE two-pair check runs per group; the openings of a failed group then go through the per-opening check on their
// weighted points (r_i is invertible mod r, so e(F'_i, g2) e(H'_i, tau_g2) = (e(F_i, g2) e(-H_i, tau_g2))^(r_i) is 1 exactly when the unweighted product is).
#pragma once
#include "bn254_pairing_batch.h"
#include "bn254_msm.h"
#include "bn254_plonk.hpp"
#include "bn254_sha256.h"

namespace bn254 {

#define KZG_OPENING_LEN 192
#define KZG_KEY_MAGIC 0x59474b42u      // "BKGY"
#define KZG_KEY_VERSION 1u
#define KZG_KEY_FLAG_G1_IDENTITY 1u
#define KZG_KEY_HDR_DWORDS 4           // magic, layout version, flags, reserved
#define KZG_KEY_G1_DWORDS (2 * BN_NL)  // g1 affine, the digits a workspace element holds (x | y)
#define KZG_KEY_REC0_DWORD (KZG_KEY_HDR_DWORDS + KZG_KEY_G1_DWORDS)
#define KZG_KEY_DWORDS (KZG_KEY_REC0_DWORD + 2 * PB_PREP_DWORDS)
#define KZG_KEY_LEN ((size_t)KZG_KEY_DWORDS * 4)
// term records of an opening (MsmTerm layout, MSM_TERM_DWORDS each) and the sums they form
//   exact:     sum 0 = H z (variable) + g1 (-y) (variable) + C (unit)
//   weighted:  sum 0 = C r + H (r z) + g1 (-r y) (variable);   sum 1 = H (-r) (variable)
#define KZG_TERMS_EXACT 3
#define KZG_TERMS_RLC 4
#define KZG_MAX_LAUNCH ((size_t)1 << 18)
// identity flags of the two G1 points in a PENDING status byte between the G1 walk and k_kzg_ident, which moves them to VP_IDENT (the pairing batch keeps
// identities there, not in status bits)
#define KZG_ST_F_INF BN254_ST_LINF
#define KZG_ST_H_INF BN254_ST_LINF2

inline MsmShape kzg_msm_shape(bool weighted) {
  MsmShape sh;
  std::memset(&sh, 0, sizeof sh);
  if (!weighted) {
    sh.n_sums = 1; sh.n_var[0] = 2; sh.var_term[0][0] = 0; sh.var_term[0][1] = 1; sh.n_unit[0] = 1; sh.unit_term[0][0] = 2;
  } else {
    sh.n_sums = 2; sh.n_var[0] = 3; sh.var_term[0][0] = 0; sh.var_term[0][1] = 1; sh.var_term[0][2] = 2; sh.n_var[1] = 1; sh.var_term[1][0] = 3;
  }
  return sh;
}

BN_HD bool kzg_key_header_ok(const int32_t* key) {
  return (uint32_t)key[0] == KZG_KEY_MAGIC && (uint32_t)key[1] == KZG_KEY_VERSION && pb_records_ok(key + KZG_KEY_REC0_DWORD, 3u);
}
// the identity bits the key contributes to VP_IDENT: bit 1 g2, bit 3 tau_g2
BN_HD uint32_t kzg_key_ident(const int32_t* key) {
  const int32_t* r0 = key + KZG_KEY_REC0_DWORD;
  return (((uint32_t)r0[2] & PB_PREP_FLAG_IDENTITY) ? 2u : 0u) | (((uint32_t)r0[PB_PREP_DWORDS + 2] & PB_PREP_FLAG_IDENTITY) ? 8u : 0u);
}

// ---- scalars: Fr on 8 x 32-bit words (bn254_rlc.h) ---------------------------------------------------------------------------------------------------------------
BN_HD Fr8 kzg_fr_neg(const Fr8& a) {   // a < r
  uint32_t o = 0;
  Fr8 r; uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { o |= a.w[i]; const uint64_t x = (uint64_t)bn_r_word(i) - a.w[i] - br; r.w[i] = (uint32_t)x; br = (x >> 32) & 1; }
#pragma unroll
  for (int i = 0; i < 8; i++) r.w[i] = o ? r.w[i] : 0u;
  return r;
}
// one term record: the affine point as reduced digits, the GLV halves of the canonical scalar k, the flag byte (bit 0: `dead`, bits 1 / 2 the halves' signs)
BN_HD void kzg_put_var(int32_t* t, uint8_t* fl, const G1Aff& p, const Fr8& k, bool dead) {
  const Fp cx = fp_reduce(fp_norm(p.x)), cy = fp_reduce(fp_norm(p.y));
#pragma unroll
  for (int i = 0; i < BN_NL; i++) { t[i] = cx.v[i]; t[BN_NL + i] = cy.v[i]; }
  bn254host::FrM kc;
#pragma unroll
  for (int i = 0; i < 4; i++) kc.l[i] = (uint64_t)k.w[2 * i] | ((uint64_t)k.w[2 * i + 1] << 32);
  const bn254host::Glv g = bn254host::glv_decompose(kc);
  t[18] = (int32_t)(uint32_t)g.k1[0]; t[19] = (int32_t)(uint32_t)(g.k1[0] >> 32); t[20] = (int32_t)(uint32_t)g.k1[1]; t[21] = (int32_t)(uint32_t)(g.k1[1] >> 32);
  t[22] = (int32_t)(uint32_t)g.k2[0]; t[23] = (int32_t)(uint32_t)(g.k2[0] >> 32); t[24] = (int32_t)(uint32_t)g.k2[1]; t[25] = (int32_t)(uint32_t)(g.k2[1] >> 32);
  *fl = (uint8_t)((dead ? 1 : 0) | (g.neg1 ? 2 : 0) | (g.neg2 ? 4 : 0));
}
BN_HD void kzg_put_unit(int32_t* t, uint8_t* fl, const G1Aff& p, bool dead) {
  const Fp cx = fp_reduce(fp_norm(p.x)), cy = fp_reduce(fp_norm(p.y));
#pragma unroll
  for (int i = 0; i < BN_NL; i++) { t[i] = cx.v[i]; t[BN_NL + i] = cy.v[i]; }
#pragma unroll
  for (int i = 18; i < MSM_TERM_DWORDS; i++) t[i] = 0;
  *fl = (uint8_t)(dead ? 1 : 0);
}

// ---- the loader of one opening -------------------------------------------------------------------------------------------------------------------------------
// rec: the opening; key: the key's dwords, header checked by the caller; strict: BN254_FLAG_STRICT_SCALARS; wgt: null (exact) or the opening's weight, four
// little-endian words, odd.  terms / flags: the opening's KZG_TERMS_EXACT or KZG_TERMS_RLC records.  In the exact form -H goes to vp_p(1) of the workspace here; in the
// weighted form the walk's second sum does.  Returns the decided error, or BN254_ST_PENDING (| KZG_ST_H_INF: H is the identity).  The order is the definition's: strict
// scalars, then the points in record order (a coordinate >= p before the curve equation).
template <class W>
BN_HD int kzg_load_opening(W& w, const uint8_t* rec, bool aligned, const int32_t* key, bool strict, const uint32_t* wgt, int32_t* terms, uint8_t* flags) {
  const int n_terms = wgt ? KZG_TERMS_RLC : KZG_TERMS_EXACT;
  int err = 0;
  Fr8 z, y;
  pb_field_words(z.w, rec + 128, aligned); pb_field_words(y.w, rec + 160, aligned);
  if (strict && (words_ge(z.w, BN_R_WORDS) || words_ge(y.w, BN_R_WORDS))) err = BN254_ST_NOT_MEMBER;
  G1Aff C, H;
  bool c_zero = true, h_zero = true;
  {
    bool memb = true;
    C.x = pb_field(rec, aligned, memb, c_zero); C.y = pb_field(rec + 32, aligned, memb, c_zero);
    if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!c_zero && !g1_on_curve(C)) err = BN254_ST_NOT_ON_CURVE; }
  }
  {
    bool memb = true;
    H.x = pb_field(rec + 64, aligned, memb, h_zero); H.y = pb_field(rec + 96, aligned, memb, h_zero);
    if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!h_zero && !g1_on_curve(H)) err = BN254_ST_NOT_ON_CURVE; }
  }
  if (err) {
    // a decided opening: records the walk reads without meaning (every term dead)
    for (int k = 0; k < n_terms; k++) { for (int q = 0; q < MSM_TERM_DWORDS; q++) terms[k * MSM_TERM_DWORDS + q] = 0; flags[k] = 1; }
    return err;
  }
  G1Aff g1;
  g1.x = pb_rec_fp(key + KZG_KEY_HDR_DWORDS); g1.y = pb_rec_fp(key + KZG_KEY_HDR_DWORDS + BN_NL);
  const bool g1_zero = ((uint32_t)key[2] & KZG_KEY_FLAG_G1_IDENTITY) != 0;
  Fr8 r2, one = fr8_zero();
#pragma unroll
  for (int i = 0; i < 8; i++) r2.w[i] = bn_r2_word(i);
  one.w[0] = 1;
  // the scalars are used modulo r: x 2^256 mod r (exact for any x < 2^256), then out of the Montgomery form with the weight -- or with 1 -- as the other factor
  const Fr8 zm = fr8_mont_mul(z, r2), ym = fr8_mont_mul(y, r2);
  if (!wgt) {
    kzg_put_var(terms, flags, H, fr8_mont_mul(zm, one), h_zero);
    kzg_put_var(terms + MSM_TERM_DWORDS, flags + 1, g1, kzg_fr_neg(fr8_mont_mul(ym, one)), g1_zero);
    kzg_put_unit(terms + 2 * MSM_TERM_DWORDS, flags + 2, C, c_zero);
    w.st(vp_p(1), H.x); w.st(vp_p(1) + 1, fp_neg(H.y));
  } else {
    Fr8 r = fr8_zero();
#pragma unroll
    for (int i = 0; i < 4; i++) r.w[i] = wgt[i];
    kzg_put_var(terms, flags, C, r, c_zero);
    kzg_put_var(terms + MSM_TERM_DWORDS, flags + 1, H, fr8_mont_mul(zm, r), h_zero);
    kzg_put_var(terms + 2 * MSM_TERM_DWORDS, flags + 2, g1, kzg_fr_neg(fr8_mont_mul(ym, r)), g1_zero);
    kzg_put_var(terms + 3 * MSM_TERM_DWORDS, flags + 3, H, kzg_fr_neg(r), h_zero);
  }
  return BN254_ST_PENDING | (!wgt && h_zero ? KZG_ST_H_INF : 0);
}
// ---- batch-opening proofs: k commitments opened at one point with ONE quotient (plonk/kzg.rs::fold_proof, 46-126; bn254_kzg_verify_folded_batch) ----------------------
//   record (KZG_FOLD_LEN(k, data_len) bytes): D_0 .. D_{k-1} (x | y) | H (x | y) | z | y_0 .. y_{k-1} | data
//   gamma = SHA-256("gamma" | be32(z mod r) | D_0 .. D_{k-1} as they stand | be32(y_0 mod r) .. | data) mod r,   D = sum gamma^i D_i,   y^ = sum gamma^i y_i
//   verdict: e(D - y^ g1 + z H, g2) e(-H, tau_g2) == 1 -- the opening (D, H, z, y^) of above, so everything behind the loader is the code of above
// term records of a record and the sums they form (for k = 1 the records of an opening, in its order):
//   exact:     sum 0 = D_1 gamma .. D_{k-1} gamma^(k-1) (terms 0 .. k-2), H z (term k-1), g1 (-y^) (term k) variable, D_0 (term k+1) unit
//   weighted:  sum 0 = D_i (r gamma^i) (terms 0 .. k-1), H (r z) (term k), g1 (-r y^) (term k+1) variable;   sum 1 = H (-r) (term k+2) variable
// The largest k: the weighted shape has k + 3 variable terms, which a split launch walks in two rows each (bn254_msm.h): 2 (k + 3) <= MSM_MAX_ROWS
#define KZG_FOLD_MAX_DIGESTS 13
#define KZG_FOLD_MAX_DATA 64
#define KZG_FOLD_LEN(k, data_len) ((size_t)96 + (size_t)96 * (size_t)(k) + (size_t)(data_len))
#define KZG_FOLD_TERMS(k, weighted) ((int)(k) + ((weighted) ? 3 : 2))
static_assert(2 * (KZG_FOLD_MAX_DIGESTS + 3) <= MSM_MAX_ROWS && 2 * (KZG_FOLD_MAX_DIGESTS + 4) > MSM_MAX_ROWS && KZG_FOLD_MAX_DIGESTS + 2 <= MSM_MAX_FIXED && KZG_FOLD_MAX_DIGESTS >= 8,
              "KZG_FOLD_MAX_DIGESTS is the largest k whose two shapes plan in the split form (tests/test_kzg_fold_cpu.py walks the planner over every k)");
// records of a pass: the term records stay within what 2^18 weighted openings take
inline size_t kzg_fold_max_launch(size_t k) {
  const size_t m = (KZG_MAX_LAUNCH * 4 / (k + 2)) & ~(size_t)63;
  return m < KZG_MAX_LAUNCH ? m : KZG_MAX_LAUNCH;
}
inline MsmShape kzg_fold_msm_shape(int k, bool weighted) {
  MsmShape sh;
  std::memset(&sh, 0, sizeof sh);
  if (!weighted) {
    sh.n_sums = 1; sh.n_var[0] = k + 1; sh.n_unit[0] = 1; sh.unit_term[0][0] = (int8_t)(k + 1);
    for (int t = 0; t <= k; t++) sh.var_term[0][t] = (int8_t)t;
  } else {
    sh.n_sums = 2; sh.n_var[0] = k + 2; sh.n_var[1] = 1; sh.var_term[1][0] = (int8_t)(k + 2);
    for (int t = 0; t < k + 2; t++) sh.var_term[0][t] = (int8_t)t;
  }
  return sh;
}
// a < 2^256 -> a mod r: 2^256 < 6 r, so conditional subtractions of 4 r, 2 r and r
BN_HD Fr8 kzg_fr_canon(const uint32_t a[8]) {
  Fr8 v;
#pragma unroll
  for (int i = 0; i < 8; i++) v.w[i] = a[i];
#pragma unroll
  for (int sh = 2; sh >= 0; sh--) {
    uint32_t d[8]; uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t m = sh ? (bn_r_word(i) << sh) | (i ? bn_r_word(i - 1) >> (32 - sh) : 0u) : bn_r_word(i);
      const uint64_t x = (uint64_t)v.w[i] - m - br; d[i] = (uint32_t)x; br = (x >> 32) & 1;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) v.w[i] = br ? v.w[i] : d[i];
  }
  return v;
}
// four message bytes at p as one big-endian word
BN_HD uint32_t kzg_be_word(const uint8_t* p, bool aligned) {
  if (aligned) return __builtin_bswap32(*(const uint32_t*)p);
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}
// The transcript of one record, hashed straight from the record: no copy of the message, no block buffer.  The message is the 5-byte name and then a SOURCE of 32-bit
// words -- z mod r (8), the digests as they stand (16 k), the y_i mod r (8 k), the data with the padding byte behind it -- so message word t is the last byte of source
// word t - 2 and the first three of source word t - 1.  The 16 words of a block are built at static positions (a field of eight words starts at word 1 or 9 of a block,
// whatever k), one compression per block in a loop whose trip count is uniform over the wavefront.  h: the digest as eight big-endian words
BN_HD void kzg_fold_transcript(uint32_t h[8], const uint8_t* rec, bool aligned, int k, int data_len, const Fr8& zc) {
  const uint32_t len = 37u + 96u * (uint32_t)k + (uint32_t)data_len, nb = (len + 8u) / 64u + 1u;
  const int u_dig = 8, u_y = 8 + 16 * k, u_data = 8 + 24 * k;      // first source word of the digests, of the values, of the data
  const uint8_t* ys = rec + 96 + 64 * (size_t)k;
  const uint8_t* data = ys + 32 * (size_t)k;
  sha256_init(h);
  Fr8 cur = zc;
  uint32_t prev = 0x61u;      // 'a', the byte of the name the first word does not hold
#pragma unroll 1
  for (uint32_t b = 0; b < nb; b++) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int t = 16 * (int)b + j, u = t - 1;
      if (t == 0) { w[0] = 0x67616d6du; continue; }      // "gamm"
      if ((j & 7) == 1 && u >= u_y && u < u_data) {      // a claimed value starts here
        uint32_t yw[8];
        pb_field_words(yw, ys + 4 * (size_t)(u - u_y), aligned);
        cur = kzg_fr_canon(yw);
      }
      uint32_t s;
      if (u < u_dig || (u >= u_y && u < u_data)) s = cur.w[7 - ((j + 7) & 7)];
      else if (u < u_y) s = kzg_be_word(rec + 4 * (size_t)(u - u_dig), aligned);
      else {
        s = 0;
        const int d0 = 4 * (u - u_data);
        if (d0 <= data_len) {
#pragma unroll
          for (int e = 0; e < 4; e++) { const int d = d0 + e; s |= (d < data_len ? (uint32_t)data[d] : d == data_len ? 0x80u : 0u) << (24 - 8 * e); }
        }
      }
      w[j] = (prev << 24) | (s >> 8);
      prev = s & 0xffu;
    }
    if (b + 1 == nb) { w[14] = 0; w[15] = 8u * len; }
    sha256_compress(h, w);
  }
}
// rec: the record; k, data_len: the call's shape (uniform over a launch); the other arguments and the result as kzg_load_opening's, with KZG_FOLD_TERMS(k, wgt) term
// records.  dbg: null, or 64 bytes for the probe -- the digest gamma is reduced from, then y^ canonical (zero for a decided record).  The order is the definition's:
// strict scalars (z, then the y_i), then the points in record order, the digests before H.
template <class W>
BN_HD int kzg_fold_load_record(W& w, const uint8_t* rec, bool aligned, int k, int data_len, const int32_t* key, bool strict, const uint32_t* wgt, int32_t* terms, uint8_t* flags,
                               uint8_t* dbg) {
  const int n_terms = KZG_FOLD_TERMS(k, wgt != nullptr);
  const uint8_t* zs = rec + 64 * (size_t)(k + 1);
  const uint8_t* ys = zs + 32;
  int err = 0;
  Fr8 z;
  pb_field_words(z.w, zs, aligned);
  if (strict) {
    bool big = words_ge(z.w, BN_R_WORDS);
#pragma unroll 1
    for (int i = 0; i < k; i++) { uint32_t yw[8]; pb_field_words(yw, ys + 32 * (size_t)i, aligned); big |= words_ge(yw, BN_R_WORDS); }
    if (big) err = BN254_ST_NOT_MEMBER;
  }
  bool h_zero = true;
#pragma unroll 1
  for (int i = 0; i <= k; i++) {      // D_0 .. D_{k-1}, then H
    bool memb = true, zero = true;
    G1Aff P;
    P.x = pb_field(rec + 64 * (size_t)i, aligned, memb, zero); P.y = pb_field(rec + 64 * (size_t)i + 32, aligned, memb, zero);
    if (err == 0) { if (!memb) err = BN254_ST_NOT_MEMBER; else if (!zero && !g1_on_curve(P)) err = BN254_ST_NOT_ON_CURVE; }
    h_zero = zero;
  }
  if (dbg) for (int q = 0; q < 64; q++) dbg[q] = 0;
  if (err) {
    for (int t = 0; t < n_terms; t++) { for (int q = 0; q < MSM_TERM_DWORDS; q++) terms[t * MSM_TERM_DWORDS + q] = 0; flags[t] = 1; }
    return err;
  }
  Fr8 r2, one = fr8_zero(), r = fr8_zero();
#pragma unroll
  for (int i = 0; i < 8; i++) r2.w[i] = bn_r2_word(i);
  one.w[0] = 1;
  if (wgt) {
#pragma unroll
    for (int i = 0; i < 4; i++) r.w[i] = wgt[i];
  } else r = one;
  const Fr8 zm = fr8_mont_mul(z, r2), zc = fr8_mont_mul(zm, one);
  Fr8 gm;      // gamma, Montgomery form
  {
    uint32_t h[8];
    kzg_fold_transcript(h, rec, aligned, k, data_len, zc);
    if (dbg) for (int q = 0; q < 8; q++) { dbg[4 * q] = (uint8_t)(h[q] >> 24); dbg[4 * q + 1] = (uint8_t)(h[q] >> 16); dbg[4 * q + 2] = (uint8_t)(h[q] >> 8); dbg[4 * q + 3] = (uint8_t)h[q]; }
    Fr8 g;
#pragma unroll
    for (int i = 0; i < 8; i++) g.w[i] = h[7 - i];
#if defined(__HIP_DEVICE_COMPILE__)
    // the digest words as plain register values before the product (the rule of FrCtx::from_be32, DESIGN.md section 9: "a wrong challenge on the device")
#pragma unroll
    for (int i = 0; i < 8; i++) asm volatile("" : "+v"(g.w[i]));
#endif
    gm = fr8_mont_mul(g, r2);
  }
  // the running power of gamma (Montgomery form) is ONE value; D_i and y_i are read again from the record
  Fr8 pw = fr8_mont_mul(r2, one), yhat = fr8_zero();
#pragma unroll 1
  for (int i = 0; i < k; i++) {
    bool memb = true, zero = true;
    G1Aff P;
    P.x = pb_field(rec + 64 * (size_t)i, aligned, memb, zero); P.y = pb_field(rec + 64 * (size_t)i + 32, aligned, memb, zero);
    Fr8 y;
    pb_field_words(y.w, ys + 32 * (size_t)i, aligned);
    yhat = fr8_add(yhat, fr8_mont_mul(fr8_mont_mul(y, r2), pw));
    if (!wgt && i == 0) kzg_put_unit(terms + (size_t)(k + 1) * MSM_TERM_DWORDS, flags + k + 1, P, zero);
    else { const int t = wgt ? i : i - 1; kzg_put_var(terms + (size_t)t * MSM_TERM_DWORDS, flags + t, P, fr8_mont_mul(pw, r), zero); }
    pw = fr8_mont_mul(pw, gm);
  }
  if (dbg) { const Fr8 yc = fr8_mont_mul(yhat, one); words_to_be(dbg + 32, yc.w); }
  G1Aff H, g1;
  {
    bool memb = true, zero = true;
    H.x = pb_field(rec + 64 * (size_t)k, aligned, memb, zero); H.y = pb_field(rec + 64 * (size_t)k + 32, aligned, memb, zero);
  }
  g1.x = pb_rec_fp(key + KZG_KEY_HDR_DWORDS); g1.y = pb_rec_fp(key + KZG_KEY_HDR_DWORDS + BN_NL);
  const bool g1_zero = ((uint32_t)key[2] & KZG_KEY_FLAG_G1_IDENTITY) != 0;
  const int th = wgt ? k : k - 1;
  kzg_put_var(terms + (size_t)th * MSM_TERM_DWORDS, flags + th, H, fr8_mont_mul(zm, r), h_zero);
  kzg_put_var(terms + (size_t)(th + 1) * MSM_TERM_DWORDS, flags + th + 1, g1, kzg_fr_neg(fr8_mont_mul(yhat, r)), g1_zero);
  if (wgt) kzg_put_var(terms + (size_t)(k + 2) * MSM_TERM_DWORDS, flags + k + 2, H, kzg_fr_neg(r), h_zero);
  else { w.st(vp_p(1), H.x); w.st(vp_p(1) + 1, fp_neg(H.y)); }
  return BN254_ST_PENDING | (!wgt && h_zero ? KZG_ST_H_INF : 0);
}
// What k_kzg_ident does for one pending item (an opening, or a group of the weighted path) once its G1 points are in the workspace: the key's G2 points to vp_q(0) and
// vp_q(1) as pb_load_item_shared stores them, the identity bits of the four points to VP_IDENT.  st: the item's status byte with the KZG_ST_*_INF flags
template <class W>
BN_HD void kzg_finish_item(W& w, const int32_t* key, uint32_t st) {
  const int32_t* r0 = key + KZG_KEY_REC0_DWORD;
  for (int j = 0; j < 2; j++)
    for (int c = 0; c < 4; c++) w.st(vp_q(j) + c, pb_rec_fp(r0 + (size_t)j * PB_PREP_DWORDS + PB_PREP_HDR_DWORDS + c * BN_NL));
  Fp m = fp_zero();
  m.v[0] = (int32_t)(kzg_key_ident(key) | ((st & KZG_ST_F_INF) ? 1u : 0u) | ((st & KZG_ST_H_INF) ? 4u : 0u));
  w.st(VP_IDENT, m);
}
// the weight of opening i of a launch: the first 128 bits of block i of the call's ChaCha20 stream, forced odd
BN_HD void kzg_weight(uint32_t out[4], const ChaChaKey& key, uint32_t i) {
  chacha20_block4(out, key, i);
  out[0] |= 1u;
}

// ---- launches (bn254_k_kzg.hip) ----------------------------------------------------------------------------------------------------------------------------------
struct KzgLoadArgs {
  const int32_t* key;            // device memory, 4-byte aligned, KZG_KEY_DWORDS dwords
  const uint8_t* openings; size_t stride; size_t n;   // n <= KZG_MAX_LAUNCH
  int32_t* ws;                   // the pairing workspace of n items
  uint8_t* status;               // n bytes, 4-byte aligned, padded to a multiple of 4 (k_g1_sum_affine ORs flags into whole words)
  int32_t* terms; uint8_t* flags;                     // n x (KZG_TERMS_EXACT | KZG_TERMS_RLC) records
  bool strict;
  bool weighted;                 // BN254_FLAG_RLC: weights from `weights` (n x 4 words, the probe) or, when that is null, from the ChaCha20 stream of wkey
  const uint32_t* weights; ChaChaKey wkey;
  // batch-opening proofs (bn254_kzg_verify_folded_batch): n_digests > 0 makes `openings` records of KZG_FOLD_LEN(n_digests, data_len) bytes or more, n at most
  // kzg_fold_max_launch(n_digests) and the term records KZG_FOLD_TERMS(n_digests, weighted) per record; dbg: null, or n x 64 bytes (the probe: digest | y^)
  // One digest without the probe is an opening with data_len bytes behind it that nothing reads (gamma^0 = 1: the fold does not depend on the transcript) and the term
  // records of an opening in an opening's order: the launcher hands such a launch to k_kzg_load, so it costs what bn254_kzg_verify_batch costs.
  int n_digests = 0, data_len = 0; uint8_t* dbg = nullptr;
};

}  // namespace bn254

hipError_t bn254_launch_kzg_load(const bn254::KzgLoadArgs& a, hipStream_t s);
// pending items of `status`: kzg_finish_item, then the status byte is BN254_ST_PENDING alone.  n items of workspace ws (openings, or the groups of a weighted launch)
hipError_t bn254_launch_kzg_ident(const int32_t* key, int32_t* ws, uint8_t* status, size_t n, hipStream_t s);
// the probe: vp_p(0), vp_p(1) of every item as 64 big-endian bytes each (zero: the identity, or an item that never reached the walk) and its two identity flags
hipError_t bn254_launch_kzg_fetch(const int32_t* ws, const uint8_t* status, size_t n, uint8_t* out_f, uint8_t* out_h, uint8_t* out_inf, hipStream_t s);
