// bn254_codec.h -- gnark's compressed point encodings, decoded by code that compiles for the host AND the device: the key loaders and
// bn254_g{1,2}_decompress (bn254_host.hpp, bn254_capi.hip) and k_g16_decompress (BN254_FLAG_COMPRESSED_PROOFS) run these same functions.
// Square roots, the root orderings and the flag handling are written branch-light: every candidate is computed and the flag and validity tests
// select among them, so a wavefront with mixed flags and mixed residuosity runs one path.  Non-residues are detected exactly (the candidate root is
// squared and compared); nothing assumes a root exists.
//
// Restates (paths relative to the reference's verifier/src): converter.rs:23-43 (flags), :62-76 (compressed G1), :113-133 (compressed G2).
#pragma once
#include "bn254_curve.h"

namespace bn254 {

enum { DEC_OK = 0, DEC_MALFORMED = 1 };

BN_HD bool fp_is_large(const Fp& a) {  // canonical value > (p-1)/2
  uint32_t w[8]; fp_to_words(w, a);
  bool ge = words_ge(w, BN_P_HALF_WORDS);
  bool eq = true;
#pragma unroll
  for (int i = 0; i < 8; i++) eq &= (w[i] == BN_P_HALF_WORDS[i]);
  return ge && !eq;
}
BN_HD int fp_cmp_canon(const Fp& a, const Fp& b) {  // -1 / 0 / 1 on the canonical values
  uint32_t x[8], y[8]; fp_to_words(x, a); fp_to_words(y, b);
  int r = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r = (x[i] != y[i]) ? (x[i] < y[i] ? -1 : 1) : r;   // the most significant differing word decides
  return r;
}
BN_HD bool fp_sqrt(Fp& out, const Fp& a) {  // p = 3 mod 4; out is meaningful only when a root exists
  Fp r = fp_pow_bits(fp_reduce(fp_norm(a)), BN_EXP_SQRT_BITS, BN_EXP_SQRT_NBITS);
  const bool ok = fp_eq(fp_sqr(r), a);
  out = r;
  return ok;
}
BN_HD Fp2 fp2_pow_bits(const Fp2& a, const uint8_t* bits, int nbits) {  // bits[0] = leading 1; public exponent: the branch is wave-uniform
  Fp2 acc = a;
  for (int i = 1; i < nbits; i++) { acc = fp2_sqr(acc); if (bits[i]) acc = fp2_mul(acc, a); }
  return acc;
}
// square root in Fp2 = Fp[i]/(i^2+1), p = 3 mod 4 (complex method); which root comes back is unspecified; out is meaningful only when a root exists.
// Both candidates (alpha = -1: i x0; otherwise (1 + alpha)^((p-1)/2) x0) are formed and selected, and the result is squared back, so a non-residue
// (a0 = -1, or any candidate that does not square to a) is refused whatever path it took.
BN_HD bool fp2_sqrt(Fp2& out, const Fp2& a) {
  const bool zero = fp2_is_zero(a);
  Fp2 a1 = fp2_pow_bits(a, BN_EXP_PM3O4_BITS, BN_EXP_PM3O4_NBITS);
  Fp2 alpha = fp2_mul(fp2_sqr(a1), a);
  Fp2 a0 = fp2_mul(fp2_conj(alpha), alpha);
  Fp2 minus_one; minus_one.c0 = fp_neg(fp_one()); minus_one.c1 = fp_zero();
  const bool nonres = fp2_eq(a0, minus_one);
  Fp2 x0 = fp2_mul(a1, a);
  Fp2 ix0; ix0.c0 = fp_neg(x0.c1); ix0.c1 = x0.c0;
  Fp2 b = fp2_pow_bits(fp2_add(alpha, fp2_one()), BN_EXP_PM1O2_BITS, BN_EXP_PM1O2_NBITS);
  Fp2 r = fp2_select(fp2_eq(alpha, minus_one), ix0, fp2_mul(b, x0));
  r = fp2_select(zero, fp2_zero(), r);
  const bool ok = zero || (!nonres && fp2_eq(fp2_sqr(r), a));
  out = r;
  return ok;
}
BN_HD bool fp2_lex_large(const Fp2& y) {  // gnark's LexicographicallyLargest
  const bool z = fp_is_zero(y.c1), l0 = fp_is_large(y.c0), l1 = fp_is_large(y.c1);
  return z ? l0 : l1;
}

// ---------------------------------------------------------------- gnark codecs on words
// w: the 32 bytes of a compressed coordinate as words_from_be reads them -- w[7] holds bytes 0..3, so the flag (converter.rs:23-43) is its top two bits:
// 0b00 panics (MALFORMED), 0b01 infinity (the rest must be zero), 0b10 / 0b11 the smaller / larger root.  x is silently reduced mod p.
BN_HD Fp dec_x_words(const uint32_t w[8], uint32_t* flag, bool* rest_zero) {
  uint32_t t[8];
#pragma unroll
  for (int i = 0; i < 8; i++) t[i] = w[i];
  *flag = t[7] >> 30;
  t[7] &= 0x3fffffffu;
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) any |= t[i];
  *rest_zero = any == 0;
  return fp_from_words(t);   // reduces any 256-bit value mod p
}
// converter.rs:62-76 (unchecked): y = sqrt(x^3+3), flag 10 -> smaller root, 11 -> larger.  The infinity flag falls through with x = 0, and 3 is a
// non-residue mod p, so it ends in InvalidPoint (a panic in the reference): every flag below 0b10 is MALFORMED.  o is meaningful only on success.
BN_HD bool dec_g1_words(G1Aff& o, const uint32_t w[8]) {
  uint32_t flag; bool rest_zero;
  const Fp x = dec_x_words(w, &flag, &rest_zero);
  Fp y = fp_zero();
  const bool has = fp_sqrt(y, fp_add(fp_mul(fp_sqr(x), x), fp_from_limbs(BN_THREE)));
  const Fp ny = fp_neg(y);
  const bool swap = fp_cmp_canon(y, ny) > 0;
  const Fp lo = fp_select(swap, ny, y), hi = fp_select(swap, y, ny);
  const bool ok = flag >= 2 && has;
  o.x = x;
  o.y = fp_select(flag == 3, hi, lo);
  return ok;
}
// converter.rs:113-133 (unchecked), x = w0 + w1 i with the flag in w1.  mode 0 (reference): the two roots are ordered by the real part c0 alone, as the
// pinned `bn` does, flag 10 -> first; mode 1 (gnark): flag 10 -> lexicographically smallest.  The infinity flag yields the G2 GENERATOR
// (AffineG2::one(), converter.rs:122-124) when the rest of the first 32 bytes is zero; the second 32 bytes are not looked at then.  o is meaningful only on success.
BN_HD bool dec_g2_words(G2Aff& o, const uint32_t w1[8], const uint32_t w0[8], int mode) {
  uint32_t flag; bool rest_zero;
  Fp2 x;
  x.c1 = dec_x_words(w1, &flag, &rest_zero);
  x.c0 = fp_from_words(w0);
  Fp2 y = fp2_zero();
  const bool has = fp2_sqrt(y, fp2_add(fp2_mul(fp2_sqr(x), x), g2_twist_b()));
  const Fp2 ny = fp2_neg(y);
  const bool y_first = (mode == 0) ? (fp_cmp_canon(y.c0, ny.c0) < 0) : !fp2_lex_large(y);
  const Fp2 ys = fp2_select((flag == 2) == y_first, y, ny);
  const bool inf = flag == 1;
  const Fp2 gx = fp2_from_limbs(BN_G2_GEN[0], BN_G2_GEN[1]), gy = fp2_from_limbs(BN_G2_GEN[2], BN_G2_GEN[3]);
  const bool ok = flag >= 2 ? has : (inf && rest_zero);
  o.x = fp2_select(inf, gx, x);
  o.y = fp2_select(inf, gy, ys);
  return ok;
}
// the byte forms (big-endian, flag in the first byte): DEC_OK / DEC_MALFORMED
BN_HD int dec_g1_compressed(G1Aff& o, const uint8_t* b32) { uint32_t w[8]; words_from_be(w, b32); return dec_g1_words(o, w) ? DEC_OK : DEC_MALFORMED; }
BN_HD int dec_g2_compressed(G2Aff& o, const uint8_t* b64, int mode) {
  uint32_t w1[8], w0[8]; words_from_be(w1, b64); words_from_be(w0, b64 + 32);
  return dec_g2_words(o, w1, w0, mode) ? DEC_OK : DEC_MALFORMED;
}

// ---------------------------------------------------------------- one compressed Groth16 proof (BN254_FLAG_COMPRESSED_PROOFS)
// in: the 32 dwords of a record A (32) | B (64: x.c1 | x.c0, flag in the first byte) | C (32) as they lie in memory (little-endian dwords of the byte
// string); out: the 64 dwords of the raw record A (64) | B (128: x.c1 | x.c0 | y.c1 | y.c0) | C (64) that bn254_g1_decompress(A, checked=0) |
// bn254_g2_decompress(B, BN254_VK_GNARK, checked=0) | bn254_g1_decompress(C, checked=0) produce.  Proof points always use gnark's root order,
// whatever mode the key was prepared with.  Returns false if any of the three does not decompress; out is then all ones: A.x >= p, which the raw
// loader answers with NOT_MEMBER at its first test, so the proof is no longer pending and contributes the neutral element to its RLC group.
BN_HD void g16_be_words(uint32_t w[8], const uint32_t* mem) {   // words_from_be on 8 dwords of a byte string
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = __builtin_bswap32(mem[7 - i]);
}
BN_HD void g16_put_fp(uint32_t* mem, const Fp& a, bool ok) {     // fp_to_be into 8 dwords of a byte string; all ones unless ok
  uint32_t w[8]; fp_to_words(w, a);
#pragma unroll
  for (int i = 0; i < 8; i++) mem[7 - i] = ok ? __builtin_bswap32(w[i]) : 0xffffffffu;
}
BN_HD bool g16_decompress_record(const uint32_t in[32], uint32_t out[64]) {
  uint32_t w1[8], w0[8];
  G1Aff a, c; G2Aff b;
  g16_be_words(w1, in);
  const bool ok_a = dec_g1_words(a, w1);
  g16_be_words(w1, in + 8); g16_be_words(w0, in + 16);
  const bool ok_b = dec_g2_words(b, w1, w0, 1);
  g16_be_words(w1, in + 24);
  const bool ok_c = dec_g1_words(c, w1);
  const bool ok = ok_a && ok_b && ok_c;
  g16_put_fp(out, a.x, ok); g16_put_fp(out + 8, a.y, ok);
  g16_put_fp(out + 16, b.x.c1, ok); g16_put_fp(out + 24, b.x.c0, ok); g16_put_fp(out + 32, b.y.c1, ok); g16_put_fp(out + 40, b.y.c0, ok);
  g16_put_fp(out + 48, c.x, ok); g16_put_fp(out + 56, c.y, ok);
  return ok;
}

}  // namespace bn254
