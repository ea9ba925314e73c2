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
};

}  // namespace bn254

hipError_t bn254_launch_kzg_load(const bn254::KzgLoadArgs& a, hipStream_t s);
// pending items of `status`: kzg_finish_item, then the status byte is BN254_ST_PENDING alone.  n items of workspace ws (openings, or the groups of a weighted launch)
hipError_t bn254_launch_kzg_ident(const int32_t* key, int32_t* ws, uint8_t* status, size_t n, hipStream_t s);
// the probe: vp_p(0), vp_p(1) of every item as 64 big-endian bytes each (zero: the identity, or an item that never reached the walk) and its two identity flags
hipError_t bn254_launch_kzg_fetch(const int32_t* ws, const uint8_t* status, size_t n, uint8_t* out_f, uint8_t* out_h, uint8_t* out_inf, hipStream_t s);
