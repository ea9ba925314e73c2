// bn254_vkprep.h -- the per-key work of bn254_groth16_vk_prepare_batch, one function per lane, compiled for the device (bn254_k_vkprep.hip) AND for the host
// (bn254_dbg_g16_vk_prepare_batch with device -1, the CPU tests): the way bn254_keys.h and bn254_sha256.h serve their kernels and their host probes.
//   vkp_dec_g1 / vkp_dec_g2   one compressed point -> canonical digits and an ok byte (dec_g1_words / dec_g2_words of bn254_codec.h)
//   vkp_fold                  one key: did every point decode; the mode's negations; the arguments of the two line tables and of e(alpha, b)
//   vkp_line_table            one G2 argument -> its 88 affine line steps, by a projective walk and ONE inversion
// Every index comes from the host's scan of the key bytes (bn254_host.hpp::scan_g16_vk): nothing here reads a count or an offset from key material.
#pragma once
#include "bn254_codec.h"
#include "bn254_pairing.h"
#include "bn254_kernels.h"

namespace bn254 {

#define VKP_G1_DWORDS (2 * BN_NL)                          // affine G1 point: x | y, canonical digits
#define VKP_G2_DWORDS (4 * BN_NL)                          // affine G2 point: x.c0 | x.c1 | y.c0 | y.c1
#define VKP_TAB_DWORDS (BN_ATE_STEPS * FIXED_LINE_DWORDS)  // one line table
#define VKP_G2_PER_KEY 5                                   // beta, gamma, delta and the two points of the commitment key
#define VKP_G1_FIXED 3                                     // alpha, beta1, delta1; K follows

// where the G1 points of a key lie among the pass's: alpha, beta1, delta1, K[0 .. count - 4]
struct VkpKey { uint32_t g1_first, g1_count; };

BN_HD void vkp_put_fp(int32_t* o, const Fp& a) {
  const Fp c = fp_reduce(fp_norm(a));
#pragma unroll
  for (int i = 0; i < BN_NL; i++) o[i] = c.v[i];
}
BN_HD void vkp_put_fp2(int32_t* o, const Fp2& a) { vkp_put_fp(o, a.c0); vkp_put_fp(o + BN_NL, a.c1); }
BN_HD Fp2 vkp_get_fp2(const int32_t* p) { return fp2_from_limbs(p, p + BN_NL); }
BN_HD void vkp_put_g2(int32_t* o, const G2Aff& q) { vkp_put_fp2(o, q.x); vkp_put_fp2(o + 2 * BN_NL, q.y); }
BN_HD G2Aff vkp_get_g2(const int32_t* p) { G2Aff q; q.x = vkp_get_fp2(p); q.y = vkp_get_fp2(p + 2 * BN_NL); return q; }
BN_HD void vkp_put_be(uint8_t* be32, const Fp& a) { uint32_t w[8]; fp_to_words(w, a); words_to_be(be32, w); }
BN_HD G1Aff vkp_g1_generator() { G1Aff g; g.x = fp_one(); g.y = fp_add(fp_one(), fp_one()); return g; }
BN_HD G2Aff vkp_g2_generator() { G2Aff g; g.x = fp2_from_limbs(BN_G2_GEN[0], BN_G2_GEN[1]); g.y = fp2_from_limbs(BN_G2_GEN[2], BN_G2_GEN[3]); return g; }

// src: the 32 (64) bytes of the compressed point as dwords of the byte string
BN_HD void vkp_dec_g1(const uint32_t* src, int32_t* out, uint8_t* ok) {
  uint32_t w[8];
  g16_be_words(w, src);
  G1Aff p;
  const bool good = dec_g1_words(p, w);
  vkp_put_fp(out, p.x); vkp_put_fp(out + BN_NL, p.y);
  *ok = good ? 1 : 0;
}
BN_HD void vkp_dec_g2(const uint32_t* src, int mode, int32_t* out, uint8_t* ok) {
  uint32_t w1[8], w0[8];
  g16_be_words(w1, src); g16_be_words(w0, src + 8);
  G2Aff q;
  const bool good = dec_g2_words(q, w1, w0, mode);
  vkp_put_g2(out, q);
  *ok = good ? 1 : 0;
}

// Key j of the pass.  It loads iff all of its points decoded; then, as prepare_g16 (bn254_host.hpp): mode 0 pairs L with gamma, C with -delta and alpha with -beta,
// mode 1 L with -gamma, C with -delta and alpha with beta.  A key that did not load goes on with the generators in place of its points, so that the lanes after this
// one compute on curve points whatever the bytes were; what they produce for it is discarded.
// targ: 2 m G2 points (the arguments of the key's two tables), barg: m G2 points, pair_g1 / pair_g2: the operands of e(alpha, b) as the pairing probe reads them
// (64 bytes x | y and 128 bytes x.c1 | x.c0 | y.c1 | y.c0, big-endian)
BN_HD void vkp_fold(uint32_t j, const VkpKey* keys, const uint8_t* ok1, const uint8_t* ok2, const int32_t* g1pts, const int32_t* g2pts, int mode, uint8_t* key_ok,
                    int32_t* targ, int32_t* barg, uint8_t* pair_g1, uint8_t* pair_g2) {
  const VkpKey k = keys[j];
  bool good = true;
  for (uint32_t i = 0; i < k.g1_count; i++) good &= ok1[(size_t)k.g1_first + i] != 0;
  for (int i = 0; i < VKP_G2_PER_KEY; i++) good &= ok2[(size_t)j * VKP_G2_PER_KEY + i] != 0;
  G1Aff alpha = vkp_g1_generator();
  G2Aff beta = vkp_g2_generator(), gamma = beta, delta = beta;
  if (good) {
    const int32_t* a = g1pts + (size_t)k.g1_first * VKP_G1_DWORDS;
    alpha.x = fp_from_limbs(a); alpha.y = fp_from_limbs(a + BN_NL);
    const int32_t* q = g2pts + (size_t)j * VKP_G2_PER_KEY * VKP_G2_DWORDS;
    beta = vkp_get_g2(q); gamma = vkp_get_g2(q + VKP_G2_DWORDS); delta = vkp_get_g2(q + 2 * VKP_G2_DWORDS);
  }
  const G2Aff g = mode == 0 ? gamma : g2_neg(gamma);
  const G2Aff d = g2_neg(delta);
  const G2Aff b = mode == 0 ? g2_neg(beta) : beta;
  vkp_put_g2(targ + (size_t)(2 * j) * VKP_G2_DWORDS, g);
  vkp_put_g2(targ + (size_t)(2 * j + 1) * VKP_G2_DWORDS, d);
  vkp_put_g2(barg + (size_t)j * VKP_G2_DWORDS, b);
  uint8_t* p1 = pair_g1 + (size_t)j * 64;
  vkp_put_be(p1, alpha.x); vkp_put_be(p1 + 32, alpha.y);
  uint8_t* p2 = pair_g2 + (size_t)j * 128;
  vkp_put_be(p2, b.x.c1); vkp_put_be(p2 + 32, b.x.c0); vkp_put_be(p2 + 64, b.y.c1); vkp_put_be(p2 + 96, b.y.c0);
  key_ok[j] = good ? 1 : 0;
}

// The line table of q (fixed_line_table's values) without an inversion per step.  The walk is the projective one of the Miller loop (g2_double_step / g2_add_step,
// then psi(q) and -psi^2(q)); its line l = r0 yP + r1 xP w + r2 w^3 is r0 times the affine line yP + m xP w + c w^3 of the same step (doubling: r0 = -2YZ, r1 = 3X^2,
// r2 = 3b'Z^2 - Y^2 against m = -3x^2 / 2y, c = (y^2 - 3b') / 2y on the curve; addition: r0 = X - x_Q Z, r1 = -(Y - y_Q Z), r2 = x_Q (Y - y_Q Z) - y_Q (X - x_Q Z)
// against m = -lambda, c = lambda x_Q - y_Q), so m = r1 / r0 and c = r2 / r0, and r0 vanishes exactly where the affine step has no slope (2 y_T = 0, x_T = x_Q).
// Forward, step s writes r0_s | r1_s a_{s-1} | r2_s a_{s-1} into its slot, a_s = r0_0 ... r0_s the running product (Montgomery's trick with the prefix folded into
// the numerators: nothing beside the table is stored).  Backward, with i_s = 1 / a_s: m_s = (r1_s a_{s-1}) i_s, c_s = (r2_s a_{s-1}) i_s, i_{s-1} = i_s r0_s -- one
// Fp2 inversion for the 88 steps.  The digits stored are canonical, so the table is the host's dword for dword.
// Returns false if some r0 vanished (unreachable for a twist point: the comment above prepare_g16); the table is then NOT normalised -- nothing is divided by a
// stand-in -- and the key is refused, as the host refuses it.
BN_HD bool vkp_line_table(int32_t* tab, const G2Aff& q) {
  G2Proj t = g2_from_affine(q);
  const G2Aff nq = g2_neg(q);
  Fp2 acc = fp2_one();
  bool bad = false;
  int n = 0;
  auto emit = [&](const G2Line& l) {
    bad |= fp2_is_zero(l.r0);
    int32_t* o = tab + (size_t)n * FIXED_LINE_DWORDS;
    vkp_put_fp2(o, l.r0);
    vkp_put_fp2(o + 2 * BN_NL, fp2_mul(l.r1, acc));
    vkp_put_fp2(o + 4 * BN_NL, fp2_mul(l.r2, acc));
    acc = fp2_mul(acc, l.r0);
    n++;
  };
  for (int i = 1; i < BN_ATE_NAF_LEN; i++) {
    emit(g2_double_step(t));
    const int d = BN_ATE_NAF[i];
    if (d != 0) emit(g2_add_step(t, d > 0 ? q : nq));   // public constant: wave-uniform
  }
  emit(g2_add_step(t, g2_psi_affine(q)));
  emit(g2_add_step(t, g2_neg(g2_psi2_affine(q))));
  if (bad || n != BN_ATE_STEPS) return false;
  Fp2 inv = fp2_inv(acc);
  for (int s = BN_ATE_STEPS - 1; s >= 0; s--) {
    int32_t* o = tab + (size_t)s * FIXED_LINE_DWORDS;
    const Fp2 r0 = vkp_get_fp2(o);
    const Fp2 m = fp2_mul(vkp_get_fp2(o + 2 * BN_NL), inv);
    const Fp2 c = fp2_mul(vkp_get_fp2(o + 4 * BN_NL), inv);
    inv = fp2_mul(inv, r0);
    vkp_put_fp2(o, m); vkp_put_fp2(o + 2 * BN_NL, c); vkp_put_fp2(o + 4 * BN_NL, fp2_mul_xi(c));
  }
  return true;
}

}  // namespace bn254

// ---- the launches of one pass (bn254_k_vkprep.hip) ----------------------------------------------------------------------------------------------------------
struct VkpLaunchArgs {
  uint32_t m;                      // keys of the pass
  uint32_t n_g1;                   // compressed G1 points of the pass; its G2 points are VKP_G2_PER_KEY * m
  int mode;
  const uint32_t* g1_src;          // 8 dwords per G1 point
  const uint32_t* g2_src;          // 16 dwords per G2 point
  const bn254::VkpKey* keys;       // m
  int32_t* g1pts; uint8_t* ok1;    // n_g1 x VKP_G1_DWORDS, n_g1
  int32_t* g2pts; uint8_t* ok2;    // 5 m x VKP_G2_DWORDS, 5 m
  uint8_t* key_ok;                 // m
  int32_t* targ;                   // 2 m x VKP_G2_DWORDS
  int32_t* barg;                   // m x VKP_G2_DWORDS
  uint8_t* pair_g1; uint8_t* pair_g2;   // m x 64, m x 128
  int32_t* tabs; uint8_t* tab_ok;  // 2 m x VKP_TAB_DWORDS, 2 m
  uint8_t* gt;                     // m x 384: e(alpha, b) as the pairing probe stores it
  int32_t* ws; uint8_t* ws_status; // the pairing program's workspace for m lanes (G16_WS_BYTES_PER_PROOF each) and its m status bytes
};
// The launches of a pass on host memory, lane after lane: what bn254_dbg_g16_vk_prepare_batch(device = -1) runs and what a host build of the library (tests/hostsan)
// puts in the place of bn254_launch_vkprep.  e(alpha, b) comes from the host's own Miller loop and final exponentiation, stored as the pairing probe stores it.
inline void vkp_run_on_host(const VkpLaunchArgs& a) {
  using namespace bn254;
  const size_t m = a.m, n_g2 = m * VKP_G2_PER_KEY;
  for (size_t i = 0; i < a.n_g1; i++) vkp_dec_g1(a.g1_src + 8 * i, a.g1pts + i * VKP_G1_DWORDS, a.ok1 + i);
  for (size_t i = 0; i < n_g2; i++) vkp_dec_g2(a.g2_src + 16 * i, a.mode, a.g2pts + i * VKP_G2_DWORDS, a.ok2 + i);
  for (size_t j = 0; j < m; j++) vkp_fold((uint32_t)j, a.keys, a.ok1, a.ok2, a.g1pts, a.g2pts, a.mode, a.key_ok, a.targ, a.barg, a.pair_g1, a.pair_g2);
  for (size_t i = 0; i < 2 * m; i++) a.tab_ok[i] = vkp_line_table(a.tabs + i * VKP_TAB_DWORDS, vkp_get_g2(a.targ + i * VKP_G2_DWORDS)) ? 1 : 0;
  for (size_t j = 0; j < m; j++) {
    uint32_t w[8];
    G1Aff p;
    words_from_be(w, a.pair_g1 + 64 * j); p.x = fp_from_words(w);
    words_from_be(w, a.pair_g1 + 64 * j + 32); p.y = fp_from_words(w);
    const Fp12 t = final_exponentiation(miller_loop<0>(p, vkp_get_g2(a.barg + j * VKP_G2_DWORDS), nullptr, nullptr));
    const Fp2 k[6] = {K0(t), K2(t), K4(t), K1(t), K3(t), K5(t)};     // the probe's byte order (k_dbg_store): tower order, big-endian
    for (int s = 0; s < 6; s++) { vkp_put_be(a.gt + 384 * j + 64 * s, k[s].c0); vkp_put_be(a.gt + 384 * j + 64 * s + 32, k[s].c1); }
  }
}
#define VKP_NUM_EVENTS 6           // before | G1 decode | G2 decode | fold | line tables | pairing
// ev: VKP_NUM_EVENTS timed events recorded around the five stages, or nullptr
hipError_t bn254_launch_vkprep(const VkpLaunchArgs& a, hipStream_t s, hipEvent_t* ev);
