// bn254_coop12.hip -- the cooperative layout for SMALL batches: TWELVE lanes per proof.
//
// A first generation (retired) spread a proof over six lanes, one Fp2 coefficient of every Fp12 value per lane: a batch of
// 4096 proofs was 410 wavefronts on 1024 SIMDs, and the time of the one launch one wavefront's serial instruction stream.  Here every Fp2 coefficient
// k_c = re + im i is split once more: lane (c, h) of a proof keeps ONE Fp number, h = 0: re, h = 1: im.  A product of two coefficients is
//     (a b)_h = a.re * b_h + a.im * (i b)_h          with  i b = (-b.im, b.re)
// so a sum of n coefficient products is one Fp dot product of 2 n terms per lane (bn254_fp.h::fp_dot: 162 n + 81 multiply-adds against
// 243 n + 162 of the Karatsuba form a six-lane layout runs), and the first operand is fetched whole while the second is fetched as the pair
// (b_h, (i b)_h): from the value itself and from an "i-image" the operation publishes first.  No exchange of partial products is needed.
// Five proofs per wavefront (lanes 60..63 idle): 4096 proofs are 820 wavefronts -- still one per SIMD -- with about 0.62 of the multiply-adds.
//
// LDS image per wavefront: img[slot][lane][12 dwords] (one Fp = 9 digits + 3 pad: three ds_read_b128; 12 * lane mod 64 puts 16 consecutive lanes
// on disjoint 4-bank groups), 13 slots = 39 KB, so FOUR wavefronts share a CU's 160 KB (the six-lane image was 66.5 KB: two).  Slots hold Fp12
// VALUES (slot numbers = the workspace map's, the final exponentiation is the same program template as everywhere else); "half h of coefficient i of value a"
// is a read at (a, group base + 2 i + h).
//
// Lock-step: a wavefront executes its LDS instructions in order, every operation reads all of its inputs before it writes
// its output slot.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <mutex>
#include "bn254_vm.h"
#include "bn254_kernels.h"
#include "bn254_launch_ops.h"   // miller_step_table

namespace bn254 {

#define C12_STRIDE 12
#define C12_SLOT(e) (((e) - VE_F) / 12)   // VE_F 0, VE_S0 1, S1 2, S2 3, S3 4, S4 5, UT0 6, (7: scratch), UT1 8, UT2 9
#define C12_X 10     // xi-multiples of an operand
#define C12_I 11     // i-multiples of an operand
#define C12_B 7      // conj(b) of a general product
#define C12_R1 7     // G2 step: products of a round; public-input MSM: the partial sums (X, Y, Z in R1, R2, R3)
#define C12_R2 11
#define C12_R3 12
#define C12_SLOTS 13
#define C12_WAVE_DWORDS (C12_SLOTS * 64 * C12_STRIDE)
#define C12_PER_WAVE 5

typedef __attribute__((address_space(3))) int32_t c12_lds_i32;   // LDS pointers keep their address space through the out-of-line operations (ds_* instead of flat_*)
typedef int c12_v4i __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) c12_v4i c12_lds_i4;
struct Coop12 {
  c12_lds_i32* img;          // this wavefront's LDS image
  uint32_t lane, g0, c, h;   // lane in the wavefront, first lane of the proof's group (12 lanes), coefficient index, half (lanes 60..63: copies of group 4)
  __device__ __forceinline__ void put(int slot, const Fp& a) const {
    c12_lds_i4* q = (c12_lds_i4*)(img + ((size_t)slot * 64 + lane) * C12_STRIDE);
    q[0] = (c12_v4i){a.v[0], a.v[1], a.v[2], a.v[3]}; q[1] = (c12_v4i){a.v[4], a.v[5], a.v[6], a.v[7]}; q[2] = (c12_v4i){a.v[8], 0, 0, 0};
  }
  __device__ __forceinline__ Fp at(int slot, uint32_t ln) const {
    const c12_lds_i4* q = (const c12_lds_i4*)(img + ((size_t)slot * 64 + ln) * C12_STRIDE);
    const c12_v4i v0 = q[0], v1 = q[1], v2 = q[2];
    Fp a;
    a.v[0] = v0.x; a.v[1] = v0.y; a.v[2] = v0.z; a.v[3] = v0.w; a.v[4] = v1.x; a.v[5] = v1.y; a.v[6] = v1.z; a.v[7] = v1.w; a.v[8] = v2.x;
    return a;
  }
  __device__ __forceinline__ Fp own(int slot) const { return at(slot, lane); }
  __device__ __forceinline__ Fp half(int slot, uint32_t i) const { return at(slot, g0 + 2 * i + h); }            // my half of coefficient i
  __device__ __forceinline__ Fp2 coef(int slot, uint32_t i) const { Fp2 r; r.c0 = at(slot, g0 + 2 * i); r.c1 = at(slot, g0 + 2 * i + 1); return r; }
};

__device__ __forceinline__ Fp2 c12_scale(const Fp2& a, int32_t w) {  // w in {0, 1, 2}, digit-wise
  Fp2 r;
#pragma unroll
  for (int i = 0; i < BN_NL; i++) { r.c0.v[i] = a.c0.v[i] * w; r.c1.v[i] = a.c1.v[i] * w; }
  return r;
}
// the pair (b_h, (i b)_h) of a value every lane holds whole
struct C12H { Fp p, q; };
__device__ __forceinline__ C12H c12_halves(const Fp2& b, uint32_t h) { C12H r; r.p = fp_select(h != 0, b.c1, b.c0); r.q = fp_select(h != 0, b.c0, fp_neg(b.c1)); return r; }
// publish the images of the value in `slot`: xi * k (my half: 9 own -/+ partner) and / or i * k (my half: -im | re)
__device__ __forceinline__ void c12_publish_xi(const Coop12& co, int slot) {
  const Fp o = co.own(slot), pt = co.at(slot, co.lane ^ 1);
  co.put(C12_X, fp_lincomb_reduce(9, o, co.h ? 1 : -1, pt));
}
__device__ __forceinline__ void c12_publish_i(const Coop12& co, int slot) {
  const Fp pt = co.at(slot, co.lane ^ 1);
  co.put(C12_I, fp_select(co.h != 0, pt, fp_neg(pt)));
}

// ---- f <- f^2 (general squaring): r_j = sum_t w_t P_t Q_t with P from the value or its xi image (whole) and Q plain (halves) -----------------------------
//   r0 = k0 k0 + 2 xk5 k1 + 2 xk4 k2 + xk3 k3     r1 = 2 k1 k0 + 2 xk5 k2 + 2 xk4 k3             r2 = 2 k2 k0 + k1 k1 + 2 xk5 k3 + xk4 k4
//   r3 = 2 k3 k0 + 2 k2 k1 + 2 xk5 k4             r4 = 2 k4 k0 + 2 k3 k1 + k2 k2 + xk5 k5         r5 = 2 k5 k0 + 2 k4 k1 + 2 k3 k2
__constant__ int8_t C12_SQ_Q[6][4] = {{0, 1, 2, 3}, {0, 2, 3, 0}, {0, 1, 3, 4}, {0, 1, 4, 0}, {0, 1, 2, 5}, {0, 1, 2, 0}};
__constant__ int8_t C12_SQ_P[6][4] = {{0, 5, 4, 3}, {1, 5, 4, 0}, {2, 1, 5, 4}, {3, 2, 5, 0}, {4, 3, 2, 5}, {5, 4, 3, 0}};
__constant__ int8_t C12_SQ_X[6][4] = {{0, 1, 1, 1}, {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 1, 0}, {0, 0, 0, 1}, {0, 0, 0, 0}};
__constant__ int8_t C12_SQ_W[6][4] = {{1, 2, 2, 1}, {2, 2, 2, 0}, {2, 1, 2, 1}, {2, 2, 2, 0}, {2, 2, 1, 1}, {2, 2, 2, 0}};
__device__ __forceinline__ void c12_sqr(const Coop12& co, int s) {
  c12_publish_xi(co, s);
  c12_publish_i(co, s);
  const uint32_t c = co.c;
  const Fp2 p0 = c12_scale(co.coef(s, C12_SQ_P[c][0]), C12_SQ_W[c][0]);
  const Fp2 p1 = c12_scale(co.coef(C12_SQ_X[c][1] ? C12_X : s, C12_SQ_P[c][1]), C12_SQ_W[c][1]);
  const Fp2 p2 = c12_scale(co.coef(C12_SQ_X[c][2] ? C12_X : s, C12_SQ_P[c][2]), C12_SQ_W[c][2]);
  const Fp2 p3 = c12_scale(co.coef(C12_SQ_X[c][3] ? C12_X : s, C12_SQ_P[c][3]), C12_SQ_W[c][3]);
  const Fp q0 = co.half(s, C12_SQ_Q[c][0]), q1 = co.half(s, C12_SQ_Q[c][1]), q2 = co.half(s, C12_SQ_Q[c][2]), q3 = co.half(s, C12_SQ_Q[c][3]);
  const Fp j0 = co.half(C12_I, C12_SQ_Q[c][0]), j1 = co.half(C12_I, C12_SQ_Q[c][1]), j2 = co.half(C12_I, C12_SQ_Q[c][2]), j3 = co.half(C12_I, C12_SQ_Q[c][3]);
  co.put(s, fp_dot(dplus(p0.c0, q0), dplus(p0.c1, j0), dplus(p1.c0, q1), dplus(p1.c1, j1), dplus(p2.c0, q2), dplus(p2.c1, j2), dplus(p3.c0, q3), dplus(p3.c1, j3)));
}
// ---- f <- f * (d0 + d3 w + d4 w^3): r_j = k_j d0 + (xi?) k_(j-1) d3 + (xi?) k_(j-3) d4: the k whole from the value or its xi image, the d as halves ---------
// d0 in Fp (the lines of the table-driven pairs, y_P): its term is own * d0.  keep: leave f (line value 1)
__device__ __forceinline__ void c12_mul_line_fp(const Coop12& co, int s, const Fp& d0, const C12H& d3, const C12H& d4, bool keep) {
  c12_publish_xi(co, s);
  const uint32_t c = co.c;
  const Fp k = co.own(s);
  const Fp2 k1 = co.coef(c >= 1 ? s : C12_X, (c + 5) % 6), k3 = co.coef(c >= 3 ? s : C12_X, (c + 3) % 6);
  const Fp r = fp_dot(dplus(k, d0), dplus(k1.c0, d3.p), dplus(k1.c1, d3.q), dplus(k3.c0, d4.p), dplus(k3.c1, d4.q));
  co.put(s, fp_select(keep, k, r));
}
// d0 in Fp2 (the line of a variable pair).  keep as above: the own half of k_c is already in hand
__device__ __forceinline__ void c12_mul_line_fp2(const Coop12& co, int s, const C12H& d0, const C12H& d3, const C12H& d4, bool keep = false) {
  c12_publish_xi(co, s);
  const uint32_t c = co.c;
  const Fp2 k0 = co.coef(s, c);
  const Fp2 k1 = co.coef(c >= 1 ? s : C12_X, (c + 5) % 6), k3 = co.coef(c >= 3 ? s : C12_X, (c + 3) % 6);
  const Fp r = fp_dot(dplus(k0.c0, d0.p), dplus(k0.c1, d0.q), dplus(k1.c0, d3.p), dplus(k1.c1, d3.q), dplus(k3.c0, d4.p), dplus(k3.c1, d4.q));
  co.put(s, fp_select(keep, fp_select(co.h != 0, k0.c1, k0.c0), r));
}
// ---- general product d <- a * (conj?) b:  r_j = sum_t (xi if t > j) a_t b_((j - t) mod 6): xi image of a, i image of (conj?) b --------------------------------
__device__ __noinline__ void c12_mul(const Coop12 co, int d, int a, int b, bool conj_b) {
  const uint32_t c = co.c;
  c12_publish_xi(co, a);
  int bp = b;
  if (conj_b) {   // conjugation negates the odd coefficients: a plain image of conj(b) in the scratch slot
    const Fp o = co.own(b);
    co.put(C12_B, (c & 1) ? fp_neg(o) : o);
    bp = C12_B;
  }
  c12_publish_i(co, bp);
  Fp acc;
  {
    const Fp2 a0 = co.coef(0 <= (int)c ? a : C12_X, 0), a1 = co.coef(1 <= c ? a : C12_X, 1), a2 = co.coef(2 <= c ? a : C12_X, 2);
    const uint32_t i0 = (c + 6 - 0) % 6, i1 = (c + 6 - 1) % 6, i2 = (c + 6 - 2) % 6;
    const Fp q0 = co.half(bp, i0), q1 = co.half(bp, i1), q2 = co.half(bp, i2), j0 = co.half(C12_I, i0), j1 = co.half(C12_I, i1), j2 = co.half(C12_I, i2);
    acc = fp_dot(dplus(a0.c0, q0), dplus(a0.c1, j0), dplus(a1.c0, q1), dplus(a1.c1, j1), dplus(a2.c0, q2), dplus(a2.c1, j2));
  }
  {
    const Fp2 a3 = co.coef(3 <= c ? a : C12_X, 3), a4 = co.coef(4 <= c ? a : C12_X, 4), a5 = co.coef(5 <= c ? a : C12_X, 5);
    const uint32_t i3 = (c + 6 - 3) % 6, i4 = (c + 6 - 4) % 6, i5 = (c + 6 - 5) % 6;
    const Fp q3 = co.half(bp, i3), q4 = co.half(bp, i4), q5 = co.half(bp, i5), j3 = co.half(C12_I, i3), j4 = co.half(C12_I, i4), j5 = co.half(C12_I, i5);
    acc = fp_add(acc, fp_dot(dplus(a3.c0, q3), dplus(a3.c1, j3), dplus(a4.c0, q4), dplus(a4.c1, j4), dplus(a5.c0, q5), dplus(a5.c1, j5)));
  }
  co.put(d, acc);
}
// ---- Granger-Scott squarings, `count` times (pairing of coefficients and roles: bn254_tower.h::fp12_cyclo_sqr) ------------------------------------------------
__constant__ int8_t C12_CY_A[6] = {0, 2, 1, 0, 2, 1};
__constant__ int8_t C12_CY_B[6] = {3, 5, 4, 3, 5, 4};
__device__ __noinline__ void c12_cyclo_sqr_n(const Coop12 co, int d, int s, int count) {
  const uint32_t c = co.c, h = co.h;
  const bool is_s = (c == 0) | (c == 2) | (c == 4);   // lanes that compute S = xi b^2 + a^2; the others T = 2 a b (xi on it for coefficient 1)
  const int32_t lin = is_s ? -2 : 2;
  Fp k = co.own(s);
  for (int it = 0; it < count; it++) {
    const int src = it == 0 ? s : d;
    const Fp2 a = co.coef(src, C12_CY_A[c]), b = co.coef(src, C12_CY_B[c]);
    // X = u1 v1 + u2 v2 with (u1, v1, u2, v2) = (xi b, b, a, a) or (2 a, b or xi b, 0, a)
    const Fp2 xb = fp2_mul_xi(b);
    const Fp2 u1 = fp2_select(is_s, xb, c12_scale(a, 2));
    const Fp2 v1 = fp2_select(is_s | (c == 1), is_s ? b : xb, b);
    const Fp2 u2 = c12_scale(a, is_s ? 1 : 0);
    const C12H h1 = c12_halves(v1, h), h2 = c12_halves(a, h);
    const Fp X = fp_dot(dplus(u1.c0, h1.p), dplus(u1.c1, h1.q), dplus(u2.c0, h2.p), dplus(u2.c1, h2.q));
    const Fp z = fp_lincomb_reduce(3, X, lin, k);
    co.put(d, z);
    k = z;
  }
}
__device__ __noinline__ void c12_conj(const Coop12 co, int d, int s) {
  const Fp k = co.own(s);
  co.put(d, (co.c & 1) ? fp_neg(k) : k);
}
__device__ __noinline__ void c12_frob(const Coop12 co, int d, int s, int j) {
  Fp2 k = co.coef(s, co.c);
  if (j & 1) k = fp2_conj(k);
  const int32_t(*t)[2][BN_NL] = j == 1 ? BN_FROB_G1 : j == 2 ? BN_FROB_G2 : BN_FROB_G3;
  Fp2 g;
#pragma unroll
  for (int l = 0; l < BN_NL; l++) { g.c0.v[l] = t[co.c][0][l]; g.c1.v[l] = t[co.c][1][l]; }
  const C12H gh = c12_halves(g, co.h);
  co.put(d, fp_dot(dplus(k.c0, gh.p), dplus(k.c1, gh.q)));   // coefficient 0: g = 1
}
// inverse: every lane gathers the whole value and runs the one-proof-per-lane inversion; lane (c, h) keeps its half of coefficient c
__device__ __noinline__ void c12_inv(const Coop12 co, int d, int s) {
  Fp12 f;
  K0(f) = co.coef(s, 0); K1(f) = co.coef(s, 1); K2(f) = co.coef(s, 2); K3(f) = co.coef(s, 3); K4(f) = co.coef(s, 4); K5(f) = co.coef(s, 5);
  Fp12 r = fp12_inv(f);
  const uint32_t c = co.c;
  const Fp2 o = fp2_select(c == 0, K0(r), fp2_select(c == 1, K1(r), fp2_select(c == 2, K2(r), fp2_select(c == 3, K3(r), fp2_select(c == 4, K4(r), K5(r))))));
  co.put(d, fp_select(co.h != 0, o.c1, o.c0));
}
struct Coop12Ops {
  const Coop12& co;
  __device__ __forceinline__ void f12_inv(int d, int a) { c12_inv(co, C12_SLOT(d), C12_SLOT(a)); }
  __device__ __forceinline__ void f12_conj(int d, int a) { c12_conj(co, C12_SLOT(d), C12_SLOT(a)); }
  // a flagged VE_CONJ (bn254_vm.h): conj(a) b = conj(a conj(b)) and conj(a) conj(b) = conj(a b), so the conjugation of a moves to the result
  __device__ __forceinline__ void f12_mul(int d, int a, int b, bool conj_b = false) {
    c12_mul(co, C12_SLOT(d), C12_SLOT(ve_elem(a)), C12_SLOT(b), conj_b != ve_conj(a));
    if (ve_conj(a)) c12_conj(co, C12_SLOT(d), C12_SLOT(d));
  }
  __device__ __forceinline__ void f12_frob(int d, int a, int j) { c12_frob(co, C12_SLOT(d), C12_SLOT(a), j); }
  // conj(a)^(2^count) = conj(a^(2^count))
  __device__ __forceinline__ void f12_cyclo_sqr(int d, int a) { f12_cyclo_sqr_n(d, a, 1); }
  __device__ __forceinline__ void f12_cyclo_sqr_n(int d, int a, int count) {
    c12_cyclo_sqr_n(co, C12_SLOT(d), C12_SLOT(ve_elem(a)), count);
    if (ve_conj(a)) c12_conj(co, C12_SLOT(d), C12_SLOT(d));
  }
};

// ---- workspace access -----------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fp c12_ws_ld(const int32_t* ws, uint32_t n, uint32_t p, int e) {
  Fp r;
#pragma unroll
  for (int l = 0; l < BN_NL; l++) r.v[l] = ws[((size_t)e * BN_NL + l) * n + p];
  return r;
}
__device__ __forceinline__ void c12_ws_st(int32_t* ws, uint32_t n, uint32_t p, int e, const Fp& a) {
#pragma unroll
  for (int l = 0; l < BN_NL; l++) ws[((size_t)e * BN_NL + l) * n + p] = a.v[l];
}
__device__ __forceinline__ Fp2 c12_ws_ld2(const int32_t* ws, uint32_t n, uint32_t p, int e) { Fp2 r; r.c0 = c12_ws_ld(ws, n, p, e); r.c1 = c12_ws_ld(ws, n, p, e + 1); return r; }
__device__ __forceinline__ FixedLine c12_line_entry(const int32_t* entry) {   // wave-uniform table entry: scalar loads
  FixedLine l;
#pragma unroll
  for (int i = 0; i < BN_NL; i++) {
    l.m.c0.v[i] = entry[i]; l.m.c1.v[i] = entry[BN_NL + i]; l.c.c0.v[i] = entry[2 * BN_NL + i]; l.c.c1.v[i] = entry[3 * BN_NL + i];
    l.xc.c0.v[i] = entry[4 * BN_NL + i]; l.xc.c1.v[i] = entry[5 * BN_NL + i];
  }
  return l;
}
// the value in `slot` goes back to the workspace element e: lane (c, h) holds Fp number 2 c + h of it
__device__ __forceinline__ void c12_store_f12(const Coop12& co, int32_t* ws, uint32_t n, uint32_t p, int slot, int e, bool pending) {
  const Fp r = co.own(slot);
  if (pending) c12_ws_st(ws, n, p, e + 2 * (int)co.c + (int)co.h, r);
}

// the value in `slot` against a constant (12 Fp in k-order): every lane compares its own Fp number, the twelve lanes of a proof vote
__device__ __forceinline__ bool c12_eq_const(const Coop12& co, int slot, const int32_t* __restrict__ target, uint32_t pl) {
  Fp t;
#pragma unroll
  for (int l = 0; l < BN_NL; l++) t.v[l] = target[(2 * (int)co.c + (int)co.h) * BN_NL + l];
  BN_SETB(t, 1.0, 0.5);
  const uint64_t m = __builtin_amdgcn_ballot_w64(fp_eq(co.own(slot), t));
  return ((m >> (pl * 12u)) & 0xfffull) == 0xfffull;
}

// A kernel's first lines, in two parts: where the lane sits (group pl of the wavefront, coefficient c, half h, proof p; pc: p clamped into the batch), and --
// given the proof's status byte -- whether it is still pending, the return of a wavefront with nothing pending, and the LDS image
#define C12_LANES()                                                                                           \
  extern __shared__ __attribute__((aligned(16))) int32_t c12_lds[];                                           \
  const uint32_t lane = threadIdx.x & 63;                                                                     \
  const bool act = lane < 12 * C12_PER_WAVE;                                                                  \
  const uint32_t la = act ? lane : lane - 12;             /* idle lanes shadow the last group */             \
  const uint32_t pl = la / 12, c = (la - pl * 12) >> 1, h = la & 1;                                           \
  const uint32_t p = blockIdx.x * (uint32_t)C12_PER_WAVE + pl;                                                \
  const bool live = act && p < n;                                                                             \
  const uint32_t pc = p < n ? p : n - 1
#define C12_PENDING(st)                                                                                       \
  const bool pending = live && ((st) & BN254_ST_PENDING) != 0;                                                \
  if (__builtin_amdgcn_ballot_w64(pending) == 0) return;                                                      \
  Coop12 co{(c12_lds_i32*)c12_lds, lane, pl * 12, c, h}
#define C12_PROLOGUE()                                                                                        \
  C12_LANES();                                                                                                \
  const uint8_t st = status[pc];                                                                              \
  C12_PENDING(st)

// ---- final exponentiation of VE_F (workspace) -> VE_S0 (workspace), the whole program in one launch ---------------------------------------------------------
__global__ void __launch_bounds__(64) k_coop12_final_exp(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status) {
  C12_PROLOGUE();
  co.put(C12_SLOT(VE_F), c12_ws_ld(ws, n, pc, VE_F + 2 * (int)c + (int)h));
  Coop12Ops ops{co};
  vm_final_exp_program(ops);
  c12_store_f12(co, ws, n, p, C12_SLOT(VE_S0), VE_S0, pending);
}

// ---- probe (bn254_dbg_coop12_op / bn254_dbg_verdict; tests): ONE operation on workspace values, called as the kernels of this file call it ---------------------------
// Operands: VE_F (and VE_S1: the second factor, or a line d0 + d3 w + d4 w^3 given as the Fp12 with k0 = d0, k1 = d3, k3 = d4); result: VE_S0.  op 12 is the
// comparison of the fused kernels: VE_F against `target`, the verdict to the status byte.  Five proofs per wavefront, the shadow lanes and the groups past
// the batch run along as they do in the product.
__global__ void __launch_bounds__(64) k_coop12_dbg_op(int32_t* ws, uint32_t n, uint8_t* status, int op_, int arg_, const int32_t* __restrict__ target) {
  C12_PROLOGUE();
  const int op = __builtin_amdgcn_readfirstlane(op_), arg = __builtin_amdgcn_readfirstlane(arg_);
  const int F = C12_SLOT(VE_F), S0 = C12_SLOT(VE_S0), S1 = C12_SLOT(VE_S1);
  co.put(F, c12_ws_ld(ws, n, pc, VE_F + 2 * (int)c + (int)h));
  co.put(S1, c12_ws_ld(ws, n, pc, VE_S1 + 2 * (int)c + (int)h));
  Coop12Ops ops{co};
  int res = S0;
  if (op == 0) ops.f12_mul(VE_S0, VE_F, VE_S1);
  else if (op == 1) ops.f12_mul(VE_S0, VE_F, VE_S1, true);
  else if (op == 2) ops.f12_mul(VE_S0, VE_F | VE_CONJ, VE_S1);
  else if (op == 3) { c12_sqr(co, F); res = F; }
  else if (op == 4) ops.f12_cyclo_sqr_n(VE_S0, VE_F, arg);
  else if (op == 5) ops.f12_frob(VE_S0, VE_F, arg);
  else if (op == 6) ops.f12_inv(VE_S0, VE_F);
  else if (op == 7) ops.f12_conj(VE_S0, VE_F);
  else if (op == 8 || op == 9) {
    const Fp d0 = c12_ws_ld(ws, n, pc, VE_S1);
    const Fp2 d3 = c12_ws_ld2(ws, n, pc, VE_S1 + 2), d4 = c12_ws_ld2(ws, n, pc, VE_S1 + 6);
    c12_mul_line_fp(co, F, d0, c12_halves(d3, h), c12_halves(d4, h), op == 9);
    res = F;
  } else if (op == 10) {
    const Fp2 d0 = c12_ws_ld2(ws, n, pc, VE_S1), d3 = c12_ws_ld2(ws, n, pc, VE_S1 + 2), d4 = c12_ws_ld2(ws, n, pc, VE_S1 + 6);
    c12_mul_line_fp2(co, F, c12_halves(d0, h), c12_halves(d3, h), c12_halves(d4, h));
    res = F;
  } else {
    const bool acc = c12_eq_const(co, F, target, pl);
    if (pending && c == 0 && h == 0) status[p] = acc ? BN254_ST_ACCEPT : BN254_ST_REJECT;
    return;
  }
  c12_store_f12(co, ws, n, p, res, VE_S0, pending);
}

// ---- Miller loop of the table-driven pairs only (PlonK's two-pair check): f = prod_t Miller(P_t, Q_t), then the final exponentiation ----------------------------
// One loop and one finish serve two kernels, which differ in where the line tables come from:
//   k_coop12_miller_fixed        the key of the launch: tab0 / tab1 are launch arguments, n_pairs is 1 or 2
//   k_coop12_miller_fixed_keys   the key TAKEN PER ITEM (a pass of a batch over many keys, and the groups of its BN254_FLAG_RLC form), exactly two pairs: item p belongs
//                                to key key_words[p >> key_shift] of the list (key_shift 6: a pass over slots with the pass's granule -> key words; key_shift 0: one
//                                word per item, the groups of a pass, whose group g is its granule g) and takes tab0 / tab1 from that key's descriptor
// The loop is templated on the table source, which hands out (m, c) of a pair's entry of step s and is told when a pair's line product has been issued.
// a pointer read from memory is a generic pointer to the compiler (flat loads): the descriptors' pointers are named global
__device__ __forceinline__ const int32_t* c12_global_ptr(uint64_t bits) { return (const int32_t*)(const __attribute__((address_space(1))) int32_t*)bits; }
__device__ __forceinline__ Fp2 c12_tab_fp2(const int32_t* e) {
  Fp2 r;
#pragma unroll
  for (int i = 0; i < BN_NL; i++) { r.c0.v[i] = e[i]; r.c1.v[i] = e[BN_NL + i]; }
  return r;
}
struct C12TabMC { Fp2 m, c; };
__device__ __forceinline__ C12TabMC c12_tab_mc(const int32_t* tab, int s) {
  C12TabMC t;
  t.m = c12_tab_fp2(tab + (size_t)s * FIXED_LINE_DWORDS); t.c = c12_tab_fp2(tab + (size_t)s * FIXED_LINE_DWORDS + 2 * BN_NL);
  return t;
}
__device__ __forceinline__ int c12_next_step(int s) { return s + 1 < BN_ATE_STEPS ? s + 1 : s; }
// the key of the launch: a wavefront-uniform entry, scalar loads where the pair's product needs it
struct C12FixedUniform {
  const int32_t *tab0, *tab1;
  __device__ __forceinline__ static C12TabMC entry(const int32_t* tab, int s) { const FixedLine l = c12_line_entry(tab + (size_t)s * FIXED_LINE_DWORDS); return C12TabMC{l.m, l.c}; }
  __device__ __forceinline__ C12TabMC pair0(int s) const { return entry(tab0, s); }
  __device__ __forceinline__ C12TabMC pair1(int s) const { return entry(tab1, s); }
  __device__ __forceinline__ void after_pair0(int) {}
  __device__ __forceinline__ void after_pair1(int) {}
};
// The key of the item.  The five items of a wavefront may belong to five keys, so the tables are read at per-lane addresses (vector loads): every lane needs m and c
// of both entries whole -- c12_halves takes both components -- and leaves xi c where it is: 72 dwords per lane and step instead of the 108 of the two entries.  An
// entry of step s + 1 is requested right after the line coefficients of step s are formed from it, so it is in flight during that line product and no second copy is
// alive.  A key word >= n_keys cannot occur for a pending slot; it reads key 0 and nothing outside the descriptors.
struct C12FixedPerItem {
  const int32_t *tab0, *tab1;
  C12TabMC l0, l1;
  __device__ __forceinline__ C12FixedPerItem(const PlonkKeyDesc* desc, uint32_t n_keys, uint32_t kw) {
    static_assert(sizeof(PlonkKeyDesc) == 40 && offsetof(PlonkKeyDesc, tab0) == 16 && offsetof(PlonkKeyDesc, tab1) == 24, "the descriptor's line tables are read by position");
    const uint64_t* kd = (const uint64_t*)(desc + (kw < n_keys ? kw : 0u));
    tab0 = c12_global_ptr(kd[2]); tab1 = c12_global_ptr(kd[3]);
    l0 = c12_tab_mc(tab0, 0); l1 = c12_tab_mc(tab1, 0);
  }
  __device__ __forceinline__ C12TabMC pair0(int) const { return l0; }
  __device__ __forceinline__ C12TabMC pair1(int) const { return l1; }
  __device__ __forceinline__ void after_pair0(int s) { l0 = c12_tab_mc(tab0, c12_next_step(s)); }   // in flight during the second line product and the squaring of step s + 1
  __device__ __forceinline__ void after_pair1(int s) { l1 = c12_tab_mc(tab1, c12_next_step(s)); }   // in flight during the squaring and the first line product of step s + 1
};
// f <- f * (the line y_P + m x_P w + c w^3 of a table-driven pair): (m x_P)_h = m_h x_P and (i m x_P)_h = (i m)_h x_P, one Fp product each.  inf: P is the identity
__device__ __forceinline__ void c12_fixed_pair(const Coop12& co, int F, const Fp2& m, const Fp2& c, const Fp& px, const Fp& py, bool inf) {
  const C12H mh = c12_halves(m, co.h);
  C12H d3; d3.p = fp_mul(mh.p, px); d3.q = fp_mul(mh.q, px);
  c12_mul_line_fp(co, F, py, d3, c12_halves(c, co.h), inf);
}
// P_0 = (VE_LX, VE_LY), P_1 = (VE_CX, VE_CY) with the identity flags BN254_ST_LINF, BN254_ST_LINF2 of the status byte
template <class Src>
__device__ __forceinline__ void c12_fixed_miller(const Coop12& co, const int32_t* ws, uint32_t n, uint32_t pc, uint8_t st, const uint8_t* __restrict__ kinds, int np, Src& src) {
  const int F = C12_SLOT(VE_F);
  co.put(F, (co.c == 0 && co.h == 0) ? fp_one() : fp_zero());
  const Fp px0 = c12_ws_ld(ws, n, pc, VE_LX), py0 = c12_ws_ld(ws, n, pc, VE_LY), px1 = c12_ws_ld(ws, n, pc, VE_CX), py1 = c12_ws_ld(ws, n, pc, VE_CY);
  const bool i0 = (st & BN254_ST_LINF) != 0, i1 = (st & BN254_ST_LINF2) != 0;
  for (int s = 0; s < BN_ATE_STEPS; s++) {
    const int kind = __builtin_amdgcn_readfirstlane((int)kinds[s]);
    if (kind == 0 && s != 0) c12_sqr(co, F);
    { const C12TabMC l = src.pair0(s); c12_fixed_pair(co, F, l.m, l.c, px0, py0, i0); }
    src.after_pair0(s);
    if (np > 1) {
      { const C12TabMC l = src.pair1(s); c12_fixed_pair(co, F, l.m, l.c, px1, py1, i1); }
      src.after_pair1(s);
    }
  }
}
// final exponentiation, then the verdict in the same launch (k_g16_compare's rule: the result never reaches the workspace) or, without a target, the store of VE_S0
__device__ __forceinline__ void c12_fixed_finish(const Coop12& co, int32_t* ws, uint32_t n, uint8_t* status, uint32_t p, uint32_t pl, bool pending, const int32_t* __restrict__ target,
                                                 int reject_code) {
  Coop12Ops ops{co};
  vm_final_exp_program(ops);
  if (target) {
    const bool acc = c12_eq_const(co, C12_SLOT(VE_S0), target, pl);
    if (pending && co.c == 0 && co.h == 0) status[p] = acc ? BN254_ST_ACCEPT : (uint8_t)reject_code;
  } else c12_store_f12(co, ws, n, p, C12_SLOT(VE_S0), VE_S0, pending);
}
__global__ void __launch_bounds__(64)
k_coop12_miller_fixed(int32_t* ws, uint32_t n, uint8_t* status, const uint8_t* __restrict__ kinds, int n_pairs, const int32_t* __restrict__ tab0,
                      const int32_t* __restrict__ tab1, const int32_t* __restrict__ target, int reject_code) {
  C12_PROLOGUE();
  C12FixedUniform src{tab0, tab1};
  c12_fixed_miller(co, ws, n, pc, st, kinds, __builtin_amdgcn_readfirstlane(n_pairs), src);
  c12_fixed_finish(co, ws, n, status, p, pl, pending, target, reject_code);
}
__global__ void __launch_bounds__(64)
k_coop12_miller_fixed_keys(int32_t* ws, uint32_t n, uint8_t* status, const uint8_t* __restrict__ kinds, const uint32_t* __restrict__ key_words, uint32_t key_shift,
                           const PlonkKeyDesc* __restrict__ desc, uint32_t n_keys, const int32_t* __restrict__ target, int reject_code) {
  C12_PROLOGUE();
  C12FixedPerItem src(desc, n_keys, key_words[pc >> key_shift]);
  c12_fixed_miller(co, ws, n, pc, st, kinds, 2, src);
  c12_fixed_finish(co, ws, n, status, p, pl, pending, target, reject_code);
}

// ---- Groth16: public-input MSM, the shared Miller loop of (A, B) with the running G2 point and the two table-driven pairs, final exponentiation --------------
// The G2 step's independent Fp2 products are dealt to the six coefficient positions in ROUNDS; the two lanes of a position
// compute the two halves of its product.  T = (X, Y, Z) is kept whole by every lane.
__device__ __forceinline__ Fp2 c12_sel6(uint32_t c, const Fp2& v0, const Fp2& v1, const Fp2& v2, const Fp2& v3, const Fp2& v4, const Fp2& v5) {
  return fp2_select(c == 0, v0, fp2_select(c == 1, v1, fp2_select(c == 2, v2, fp2_select(c == 3, v3, fp2_select(c == 4, v4, v5)))));
}
__device__ __forceinline__ Fp2 c12_fp_as_fp2(const Fp& a) { Fp2 r; r.c0 = a; r.c1 = fp_zero(); return r; }
__device__ __forceinline__ Fp c12_prod(const Coop12& co, const Fp2& u, const Fp2& v) {   // my half of u v
  const C12H vh = c12_halves(v, co.h);
  return fp_dot(dplus(u.c0, vh.p), dplus(u.c1, vh.q));
}
struct C12Line { Fp2 d0, d3, d4, s1, s2, cz; };   // the variable pair's line at A; m1 X_L, m2 x_C and c1 Z_L of the two table-driven pairs (L projective)
// KEYS: the three key-side products ride in the rounds' free positions (Groth16).  Without them (the batch pairing product: variable pairs only) those positions repeat
// a neighbour's operands and s1, s2, cz are left alone; the rounds are the same code either way
template <bool KEYS>
__device__ __forceinline__ void c12_g2_double_t(const Coop12& co, G2Proj& t, const Fp& xa, const Fp& ya, const Fp2& m1, const Fp& xl, const Fp2& m2, const Fp& xc, const Fp2& c1,
                                                const Fp& zl, C12Line& out) {
  const uint32_t c = co.c;
  const Fp2 yz = fp2_add(t.y, t.z);
  // round 1: X Y, Y^2, Z^2, X^2, (Y + Z)^2, m1 xl
  co.put(C12_R1, c12_prod(co, c12_sel6(c, t.x, t.y, t.z, t.x, yz, KEYS ? m1 : yz), c12_sel6(c, t.y, t.y, t.z, t.x, yz, KEYS ? c12_fp_as_fp2(xl) : yz)));
  const Fp2 A = co.coef(C12_R1, 0), B = co.coef(C12_R1, 1), C = co.coef(C12_R1, 2), J = co.coef(C12_R1, 3), S = co.coef(C12_R1, 4);
  if constexpr (KEYS) out.s1 = co.coef(C12_R1, 5);
  const Fp2 H = fp2_sub2(S, B, C);                       // 2 Y Z
  // round 2: B H, -, b3 C, H ya, J xa, m2 xc
  const Fp2 b3 = fp2_from_limbs(BN_TWIST_3B0, BN_TWIST_3B1);
  co.put(C12_R2, c12_prod(co, c12_sel6(c, B, B, b3, H, J, KEYS ? m2 : J), c12_sel6(c, H, B, C, c12_fp_as_fp2(ya), c12_fp_as_fp2(xa), c12_fp_as_fp2(KEYS ? xc : xa))));
  const Fp2 BH = co.coef(C12_R2, 0), E = co.coef(C12_R2, 2), Hy = co.coef(C12_R2, 3), Jx = co.coef(C12_R2, 4);
  if constexpr (KEYS) out.s2 = co.coef(C12_R2, 5);
  const Fp2 F = fp2_mul_small(E, 3);
  const Fp2 BmF = fp2_sub(B, F), BF = fp2_add(B, F);
  // round 3: E^2, A (B - F), (B + F)^2, c1 zl
  co.put(C12_R3, c12_prod(co, c12_sel6(c, E, A, BF, KEYS ? c1 : E, E, E), c12_sel6(c, E, BmF, BF, KEYS ? c12_fp_as_fp2(zl) : E, E, E)));
  const Fp2 E2 = co.coef(C12_R3, 0), AX = co.coef(C12_R3, 1), BF2 = co.coef(C12_R3, 2);
  if constexpr (KEYS) out.cz = co.coef(C12_R3, 3);
  t.x = fp2_dbl(AX);
  t.y = fp2_sub(BF2, fp2_mul_small(E2, 12));
  t.z = fp2_mul_small(BH, 4);
  out.d0 = fp2_neg(Hy);
  out.d3 = fp2_mul_small(Jx, 3);
  out.d4 = fp2_sub(E, B);
}
template <bool KEYS>
__device__ __forceinline__ void c12_g2_add_t(const Coop12& co, G2Proj& t, const Fp2& qx, const Fp2& qy, const Fp& xa, const Fp& ya, const Fp2& m1, const Fp& xl, const Fp2& m2,
                                             const Fp& xc, const Fp2& c1, const Fp& zl, C12Line& out) {
  const uint32_t c = co.c;
  // round 1: yQ Z, xQ Z, -, -, -, m1 xl
  co.put(C12_R1, c12_prod(co, c12_sel6(c, qy, qx, qx, qx, qx, KEYS ? m1 : qx), c12_sel6(c, t.z, t.z, t.z, t.z, t.z, KEYS ? c12_fp_as_fp2(xl) : t.z)));
  const Fp2 O = fp2_sub(t.y, co.coef(C12_R1, 0)), L = fp2_sub(t.x, co.coef(C12_R1, 1));
  if constexpr (KEYS) out.s1 = co.coef(C12_R1, 5);
  // round 2: O^2, L^2, xQ O, L yQ, L ya, m2 xc
  co.put(C12_R2, c12_prod(co, c12_sel6(c, O, L, qx, L, L, KEYS ? m2 : L), c12_sel6(c, O, L, O, qy, c12_fp_as_fp2(ya), c12_fp_as_fp2(KEYS ? xc : ya))));
  const Fp2 Cc = co.coef(C12_R2, 0), D = co.coef(C12_R2, 1), xqO = co.coef(C12_R2, 2), Lyq = co.coef(C12_R2, 3);
  out.d0 = co.coef(C12_R2, 4);
  if constexpr (KEYS) out.s2 = co.coef(C12_R2, 5);
  // round 3: L D, Z C, X D, O xa, c1 zl
  co.put(C12_R3, c12_prod(co, c12_sel6(c, L, t.z, t.x, O, KEYS ? c1 : O, O), c12_sel6(c, D, Cc, D, c12_fp_as_fp2(xa), KEYS ? c12_fp_as_fp2(zl) : O, O)));
  const Fp2 E = co.coef(C12_R3, 0), Fz = co.coef(C12_R3, 1), G = co.coef(C12_R3, 2), Ox = co.coef(C12_R3, 3);
  if constexpr (KEYS) out.cz = co.coef(C12_R3, 4);
  const Fp2 H = fp2_sub(fp2_add(E, Fz), fp2_dbl(G));
  const Fp2 GmH = fp2_sub(G, H);
  // round 4: L H, (G - H) O, Y E, E Z     (round-1 slot reused: its values are in registers by now)
  co.put(C12_R1, c12_prod(co, c12_sel6(c, L, GmH, t.y, E, E, E), c12_sel6(c, H, O, E, t.z, E, E)));
  t.x = co.coef(C12_R1, 0);
  t.y = fp2_sub(co.coef(C12_R1, 1), co.coef(C12_R1, 2));
  t.z = co.coef(C12_R1, 3);
  out.d3 = fp2_neg(Ox);
  out.d4 = fp2_sub(xqO, Lyq);
}
__device__ __forceinline__ void c12_g2_double(const Coop12& co, G2Proj& t, const Fp& xa, const Fp& ya, const Fp2& m1, const Fp& xl, const Fp2& m2, const Fp& xc, const Fp2& c1,
                                              const Fp& zl, C12Line& out) {
  c12_g2_double_t<true>(co, t, xa, ya, m1, xl, m2, xc, c1, zl, out);
}
__device__ __forceinline__ void c12_g2_add(const Coop12& co, G2Proj& t, const Fp2& qx, const Fp2& qy, const Fp& xa, const Fp& ya, const Fp2& m1, const Fp& xl, const Fp2& m2,
                                           const Fp& xc, const Fp2& c1, const Fp& zl, C12Line& out) {
  c12_g2_add_t<true>(co, t, qx, qy, xa, ya, m1, xl, m2, xc, c1, zl, out);
}
// the variable pair alone: d0, d3, d4 of `out`
__device__ __forceinline__ void c12_g2_double_var(const Coop12& co, G2Proj& t, const Fp& xa, const Fp& ya, C12Line& out) {
  c12_g2_double_t<false>(co, t, xa, ya, t.x, xa, t.x, xa, t.x, xa, out);
}
__device__ __forceinline__ void c12_g2_add_var(const Coop12& co, G2Proj& t, const Fp2& qx, const Fp2& qy, const Fp& xa, const Fp& ya, C12Line& out) {
  c12_g2_add_t<false>(co, t, qx, qy, xa, ya, qx, xa, qx, xa, qx, xa, out);
}
__device__ __forceinline__ G1Aff c12_msm_entry(const int32_t* __restrict__ msm_tab, size_t idx) {
  const int4* e = (const int4*)(msm_tab + idx * MSM_ENTRY_DWORDS);
  int4 v0 = e[0], v1 = e[1], v2 = e[2], v3 = e[3], v4 = e[4];
  G1Aff q;
  q.x.v[0] = v0.x; q.x.v[1] = v0.y; q.x.v[2] = v0.z; q.x.v[3] = v0.w; q.x.v[4] = v1.x; q.x.v[5] = v1.y; q.x.v[6] = v1.z; q.x.v[7] = v1.w;
  q.x.v[8] = v2.x; q.y.v[0] = v2.y; q.y.v[1] = v2.z; q.y.v[2] = v2.w; q.y.v[3] = v3.x; q.y.v[4] = v3.y; q.y.v[5] = v3.z; q.y.v[6] = v3.w;
  q.y.v[7] = v4.x; q.y.v[8] = v4.y;
  return q;
}
// L = K0 + sum_i x_i K_i (groth16/verify.rs:53-63) by the twelve lanes of a proof: lane l starts from K0 (lane 0) or the identity and adds the table entries of the
// windows w = l, l + 12, ... of its proof's inputs; the twelve partial sums are then added through LDS.  The two MSM functions differ in their window loops only.
// L stays PROJECTIVE: the line of the pair (L, g') is scaled by Z_L, an Fp factor the final exponentiation removes.
__device__ __forceinline__ G1Proj c12_msm_k0(uint32_t l12, const int32_t* k0) {
  G1Proj acc = g1_identity();
  if (l12 == 0) { G1Aff K0; for (int l = 0; l < BN_NL; l++) { K0.x.v[l] = k0[l]; K0.y.v[l] = k0[BN_NL + l]; } acc = g1_from_affine(K0); }
  return acc;
}
// acc <- acc + entry where the window's digit is not zero (the mixed addition is computed either way)
__device__ __forceinline__ void c12_msm_take(G1Proj& acc, const G1Aff& entry, bool take) {
  const G1Proj nxt = g1_add_mixed(acc, entry);
  acc.x = fp_select(take, nxt.x, acc.x); acc.y = fp_select(take, nxt.y, acc.y); acc.z = fp_select(take, nxt.z, acc.z);
}
// the sum of the twelve lanes' values, to every lane: lanes 0..5: own + lane l + 6; lanes 0, 1: l, l + 2, l + 4; 0 + 1
__device__ __forceinline__ G1Proj c12_msm_tree(const Coop12& co, G1Proj acc, uint32_t l12) {
  auto publish = [&](const G1Proj& a) { co.put(C12_R1, fp_reduce(a.x)); co.put(C12_R2, fp_reduce(a.y)); co.put(C12_R3, fp_reduce(a.z)); };
  auto fetch = [&](uint32_t i) { G1Proj r; r.x = co.at(C12_R1, co.g0 + i); r.y = co.at(C12_R2, co.g0 + i); r.z = co.at(C12_R3, co.g0 + i); return r; };
  publish(acc);
  acc = g1_add(acc, fetch(l12 < 6 ? l12 + 6 : l12));          // lanes 6..11 add their own value (result unused)
  publish(acc);
  { const uint32_t b = l12 < 2 ? l12 : 0; acc = g1_add(g1_add(fetch(b), fetch(b + 2)), fetch(b + 4)); }
  publish(acc);
  acc = g1_add(fetch(0), fetch(1));
  publish(acc);
  return fetch(0);
}
// the key of the launch: MSM_FW_WINDOWS = 20 windows of 13 bits per input (bn254_fw.h)
__device__ __noinline__ G1Proj c12_public_input_msm(const Coop12 co, const uint8_t* __restrict__ in /* this proof's inputs */, int n_public, bool use_inputs,
                                                    const int32_t* __restrict__ msm_tab, const int32_t* __restrict__ k0) {
  const uint32_t l12 = 2 * co.c + co.h;
  G1Proj acc = c12_msm_k0(l12, k0);
  const int windows = use_inputs ? MSM_FW_WINDOWS * n_public : 0;
  for (int w = (int)l12; w < windows; w += 12) {
    const int sidx = w / MSM_FW_WINDOWS, wi = w - sidx * MSM_FW_WINDOWS;
    // window wi = bits 13 wi .. 13 wi + 12 of the big-endian scalar (bn254_fw.h): at most three of its bytes, byte 31 - k holding bits 8 k .. 8 k + 7
    const int bit = MSM_FW_BITS * wi, k0b = bit >> 3;
    const uint8_t* sc = in + (size_t)sidx * 32;
    const uint32_t three = (uint32_t)sc[31 - k0b] | (k0b + 1 < 32 ? (uint32_t)sc[30 - k0b] << 8 : 0u) | (k0b + 2 < 32 ? (uint32_t)sc[29 - k0b] << 16 : 0u);
    const uint32_t dig = (three >> (bit & 7)) & MSM_FW_ENTRIES;
    c12_msm_take(acc, c12_msm_entry(msm_tab, (size_t)(sidx * MSM_FW_WINDOWS + wi) * MSM_FW_ENTRIES + (dig ? dig - 1 : 0)), dig != 0);
  }
  return c12_msm_tree(co, acc, l12);
}

// The shared Miller loop, templated on where the two line tables (table 0: the pair (L, g'), table 1: the pair (C, d')) come from.  A source hands out the operands
// of a step -- m0, c0, m1 for the G2 rounds, c1 for the third line product -- and is called at four points, of which each source uses two:
//   start()          before the first step                      C12G16PerGroup: the fetches of step 0
//   enter(s)         the squaring of step s is issued           C12G16Uniform: the scalar loads of both entries of step s
//   after_rounds(s)  the G2 rounds of step s are issued         C12G16PerGroup: requests m0 / c0 / m1 of step s + 1
//   after_lines(s)   the three line products of step s are      C12G16PerGroup: requests c1 of step s + 1
// The request points are the per-group source's contract (what is alive while a step computes: see its comment); the loop never asks which source it serves.
// the key of the launch: wavefront-uniform entries, scalar loads of both at the top of the step
struct C12G16Uniform {
  const int32_t *tab0, *tab1;
  FixedLine l0, l1;
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void enter(int s) {
    l0 = c12_line_entry(tab0 + (size_t)s * FIXED_LINE_DWORDS);
    l1 = c12_line_entry(tab1 + (size_t)s * FIXED_LINE_DWORDS);
  }
  __device__ __forceinline__ const Fp2& m0() const { return l0.m; }
  __device__ __forceinline__ const Fp2& c0() const { return l0.c; }
  __device__ __forceinline__ const Fp2& m1() const { return l1.m; }
  __device__ __forceinline__ const Fp2& c1() const { return l1.c; }
  __device__ __forceinline__ void after_rounds(int) {}
  __device__ __forceinline__ void after_lines(int) {}
};
// The key of the group: the line-table dwords a lane needs of a step.  The G2 rounds multiply m of table 0 and m of table 1 at coefficient position 5 only and c of
// table 0 at position 3 (doubling) or 4 (addition) only (c12_g2_double / c12_g2_add: the operands c12_sel6 picks), so a lane fetches ONE of m, c of table 0 -- the one
// its position multiplies -- and hands it out for both; every lane needs its halves of c of table 1 for the third line product.  54 dwords per lane and step instead
// of the 72 of the two entries, in two groups that are each fetched right after their last use in the step before: no second copy is alive while a step computes.
struct C12G16PerGroup {
  const int32_t *gtab, *dtab;
  uint32_t c;
  Fp2 mc0, m1v, c1v;      // table 0: m at position 5, c elsewhere; table 1: m; table 1: c
  __device__ __forceinline__ void fetch_g2(int s) {
    mc0 = c12_tab_fp2(gtab + (size_t)s * FIXED_LINE_DWORDS + (c == 5 ? 0 : 2 * BN_NL));
    m1v = c12_tab_fp2(dtab + (size_t)s * FIXED_LINE_DWORDS);
  }
  __device__ __forceinline__ void fetch_c1(int s) { c1v = c12_tab_fp2(dtab + (size_t)s * FIXED_LINE_DWORDS + 2 * BN_NL); }
  __device__ __forceinline__ void start() { fetch_g2(0); fetch_c1(0); }
  __device__ __forceinline__ void enter(int) {}
  __device__ __forceinline__ const Fp2& m0() const { return mc0; }
  __device__ __forceinline__ const Fp2& c0() const { return mc0; }
  __device__ __forceinline__ const Fp2& m1() const { return m1v; }
  __device__ __forceinline__ const Fp2& c1() const { return c1v; }
  __device__ __forceinline__ void after_rounds(int s) { fetch_g2(c12_next_step(s)); }      // step s + 1's: in flight during the three line products
  __device__ __forceinline__ void after_lines(int s) { fetch_c1(c12_next_step(s)); }       // in flight during the squaring and the G2 rounds of step s + 1
};
// On return q is B and t the loop's final point.
template <class Src>
__device__ __forceinline__ void c12_g16_miller(const Coop12& co, const int32_t* ws, uint32_t n, uint32_t pc, const uint8_t* __restrict__ kinds, const G1Proj& Lp, Src& src, G2Aff& q,
                                               G2Proj& t) {
  const int F = C12_SLOT(VE_F);
  const uint32_t h = co.h;
  const bool l_inf = fp_is_zero(Lp.z);
  const Fp xl = Lp.x, yl = fp_select(l_inf, fp_one(), Lp.y), zl = Lp.z;
  co.put(F, (co.c == 0 && h == 0) ? fp_one() : fp_zero());
  const Fp xa = c12_ws_ld(ws, n, pc, VE_AX), ya = c12_ws_ld(ws, n, pc, VE_AY);
  const Fp xc = c12_ws_ld(ws, n, pc, VE_CX), yc = c12_ws_ld(ws, n, pc, VE_CY);
  q.x = c12_ws_ld2(ws, n, pc, VE_B); q.y = c12_ws_ld2(ws, n, pc, VE_B + 2);
  t = g2_from_affine(q);
  src.start();
  for (int s = 0; s < BN_ATE_STEPS; s++) {
    const int kind = __builtin_amdgcn_readfirstlane((int)kinds[s]);
    if (kind == 0 && s != 0) c12_sqr(co, F);
    src.enter(s);
    C12Line ln;
    if (kind == 0) {
      c12_g2_double(co, t, xa, ya, src.m0(), xl, src.m1(), xc, src.c0(), zl, ln);
    } else {
      G2Aff b = q;
      if (kind == 2) b = g2_neg(q);
      else if (kind == 3) b = g2_psi_affine(q);
      else if (kind == 4) b = g2_neg(g2_psi2_affine(q));
      c12_g2_add(co, t, b.x, b.y, xa, ya, src.m0(), xl, src.m1(), xc, src.c0(), zl, ln);
    }
    src.after_rounds(s);
    c12_mul_line_fp2(co, F, c12_halves(ln.d0, h), c12_halves(ln.d3, h), c12_halves(ln.d4, h));
    c12_mul_line_fp(co, F, yl, c12_halves(ln.s1, h), c12_halves(ln.cz, h), l_inf);      // (Y_L + m X_L w + c Z_L w^3): the line at L scaled by Z_L
    c12_mul_line_fp(co, F, yc, c12_halves(ln.s2, h), c12_halves(src.c1(), h), false);
    src.after_lines(s);
  }
}
// The whole verdict in the launch (what k_g16_subgroup and k_g16_compare do for the lane kernels).  The r-torsion test of B from the loop's final
// point (bn254_vm.h::vm_g2_ate_check: T == -psi^3(B) projectively) costs four Fp2 products: every lane holds T and B whole and computes it for itself.
__device__ __forceinline__ void c12_g16_verdict(const Coop12& co, uint8_t* status, uint32_t p, uint32_t pl, uint8_t st, bool pending, const G2Aff& q, const G2Proj& t,
                                                const int32_t* target, int inputs_match) {
  const Fp2 sx = fp2_mul(fp2_conj(q.x), frob_coeff(3, 2)), sy = fp2_neg(fp2_mul(fp2_conj(q.y), frob_coeff(3, 3)));
  const bool in_g2 = !fp2_is_zero(t.z) & fp2_eq(t.x, fp2_mul(sx, t.z)) & fp2_eq(t.y, fp2_mul(sy, t.z));
  Coop12Ops ops{co};
  vm_final_exp_program(ops);
  const bool acc = c12_eq_const(co, C12_SLOT(VE_S0), target, pl);
  uint8_t out;
  if (!in_g2) out = BN254_ST_NOT_IN_SUBGROUP;
  else if (st & 0x3f) out = st & 0x3f;                      // deferred error of C
  else if (!inputs_match) out = BN254_ST_INPUT_LEN;         // PrepareInputsFailed comes after every loader error
  else out = acc ? BN254_ST_ACCEPT : BN254_ST_REJECT;
  if (pending && co.c == 0 && co.h == 0) status[p] = out;
}
// without a target (the probe's store mode) the GT value goes to VE_S0 of the workspace instead
__global__ void __launch_bounds__(64)
k_coop12_miller_g16(int32_t* ws, uint32_t n, uint8_t* status, const uint8_t* __restrict__ kinds, const int32_t* __restrict__ tab0,
                    const int32_t* __restrict__ tab1, const uint8_t* __restrict__ inputs, int n_public, int inputs_match_key,
                    const int32_t* __restrict__ msm_tab, const int32_t* __restrict__ k0, int l_from_ws, const int32_t* __restrict__ target) {
  C12_PROLOGUE();
  // keys with many public inputs: L was computed by the wide MSM kernels (affine, in the workspace, identity flag in the status byte)
  G1Proj Lp;
  if (l_from_ws) { Lp.x = c12_ws_ld(ws, n, pc, VE_LX); Lp.y = c12_ws_ld(ws, n, pc, VE_LY); Lp.z = (st & BN254_ST_LINF) ? fp_zero() : fp_one(); }
  else Lp = c12_public_input_msm(co, inputs + (size_t)pc * (size_t)n_public * 32, n_public, inputs_match_key != 0, msm_tab, k0);
  C12G16Uniform src{tab0, tab1};
  G2Aff q;
  G2Proj t;
  c12_g16_miller(co, ws, n, pc, kinds, Lp, src, q, t);
  if (target) { c12_g16_verdict(co, status, p, pl, st, pending, q, t, target, inputs_match_key); return; }
  Coop12Ops ops{co};
  vm_final_exp_program(ops);
  c12_store_f12(co, ws, n, p, C12_SLOT(VE_S0), VE_S0, pending);
}

// ---- Groth16 over many keys, the DIRECT form (bn254_keys.h; bn254_g16_plan.h::g16_keys_form): k_coop12_miller_g16 with the key taken per PROOF --------------------
// A slot is a proof and the key belongs to the twelve-lane group: the five proofs of a wavefront may belong to five keys.  Group p reads key_index[p] and the
// descriptor of that entry with ordinary per-lane loads (all twelve lanes the same address), and every place where k_coop12_miller_g16 takes the key from its launch
// arguments -- the two line tables, K0 and the fixed-base tables, n_public with inputs_match, the target -- takes it from there.  What differs otherwise:
//   line tables   fetched per lane with vector loads (C12G16PerGroup: 54 dwords per step), step s + 1's issued while step s computes; the scalar loads
//                 of c12_line_entry need a wavefront-uniform key
//   L             over the set's BYTE-window tables (32 windows of 8 bits per input: what k_g16_prepare_keys reads); the loop bound differs per group, all LDS
//                 traffic comes after the loop
//   prologue      the two status bytes the pipeline alone cannot decide, before the early return: an index outside the list is MALFORMED whatever the record holds,
//                 and with BN254_FLAG_STRICT_SCALARS an input >= r among the key's n_public inputs is NOT_MEMBER ahead of every loader outcome
struct C12Key { const int32_t *msm_tab, *k0, *gtab, *dtab, *target; int n_public, inputs_match; };
__device__ __forceinline__ C12Key c12_key(const G16KeyDesc* __restrict__ desc, uint32_t k) {
  // the descriptor as six 64-bit words: five pointers in this order, then the two ints
  static_assert(sizeof(G16KeyDesc) == 48 && offsetof(G16KeyDesc, msm_tab) == 0 && offsetof(G16KeyDesc, k0) == 8 && offsetof(G16KeyDesc, gtab) == 16 &&
                offsetof(G16KeyDesc, dtab) == 24 && offsetof(G16KeyDesc, target) == 32 && offsetof(G16KeyDesc, n_public) == 40 && offsetof(G16KeyDesc, inputs_match) == 44,
                "c12_key reads G16KeyDesc by position");
  const uint64_t* f = (const uint64_t*)(desc + k);
  C12Key v;
  v.msm_tab = c12_global_ptr(f[0]); v.k0 = c12_global_ptr(f[1]); v.gtab = c12_global_ptr(f[2]); v.dtab = c12_global_ptr(f[3]); v.target = c12_global_ptr(f[4]);
  const uint64_t w = f[5];
  v.n_public = (int)(uint32_t)w; v.inputs_match = (int)(uint32_t)(w >> 32);
  return v;
}
// byte windows: window wi of input s = byte 31 - wi of the big-endian scalar, entry (s * 32 + wi) * 255 + digit - 1, of the 32 n_public windows of the proof's key
__device__ __noinline__ G1Proj c12_public_input_msm_keys(const Coop12 co, const uint8_t* in /* this proof's input row */, int n_public, const int32_t* tab, const int32_t* k0p) {
  const uint32_t l12 = 2 * co.c + co.h;
  const uint8_t* row = (const uint8_t*)(const __attribute__((address_space(1))) uint8_t*)in;
  const int32_t *msm_tab = c12_global_ptr((uint64_t)tab), *k0 = c12_global_ptr((uint64_t)k0p);
  G1Proj acc = c12_msm_k0(l12, k0);
  const int windows = 32 * n_public;
  for (int w = (int)l12; w < windows; w += 12) {
    const int sidx = w >> 5, wi = w & 31;
    const uint32_t dig = row[sidx * 32 + 31 - wi];
    c12_msm_take(acc, c12_msm_entry(msm_tab, (size_t)(sidx * 32 + wi) * 255 + (dig ? dig - 1 : 0)), dig != 0);
  }
  return c12_msm_tree(co, acc, l12);
}
__global__ void __launch_bounds__(64)
k_coop12_miller_g16_keys(int32_t* ws, uint32_t n, uint8_t* status, const uint8_t* __restrict__ kinds, const uint32_t* __restrict__ key_index,
                         const G16KeyDesc* __restrict__ desc, uint32_t n_keys, const uint8_t* __restrict__ inputs, size_t input_stride, int strict_scalars) {
  C12_LANES();
  const uint32_t ki = key_index[pc];
  const bool key_ok = ki < n_keys;
  const C12Key key = c12_key(desc, key_ok ? ki : 0u);
  const uint8_t* in = inputs + (size_t)pc * input_stride;
  uint8_t st = status[pc];
  {
    bool bad = false;
    if (strict_scalars)
      for (int s = (int)(2 * c + h); s < key.n_public; s += 12) { uint32_t w[8]; words_from_be(w, in + (size_t)s * 32); bad |= words_ge(w, BN_R_WORDS); }
    const bool group_bad = ((__builtin_amdgcn_ballot_w64(act && bad) >> (pl * 12u)) & 0xfffull) != 0;
    const uint8_t fixed = !key_ok ? (uint8_t)BN254_ST_MALFORMED : group_bad ? (uint8_t)BN254_ST_NOT_MEMBER : st;
    if (live && c == 0 && h == 0 && fixed != st) status[p] = fixed;
    st = fixed;
  }
  C12_PENDING(st);
  const G1Proj Lp = c12_public_input_msm_keys(co, in, key.inputs_match ? key.n_public : 0, key.msm_tab, key.k0);
  C12G16PerGroup src{key.gtab, key.dtab, c};
  G2Aff q;
  G2Proj t;
  c12_g16_miller(co, ws, n, pc, kinds, Lp, src, q, t);
  c12_g16_verdict(co, status, p, pl, st, pending, q, t, key.target, key.inputs_match);
}

// ---- the batch pairing product (bn254_pairing_batch.h): 1 .. VP_MAX_PAIRS VARIABLE pairs per item and no key, after the unchanged k_pairing_load -----------------
// bn254_vm.h::vm_miller_run_var step for step: the squaring of f once per doubling step, then for every pair j its G2 step on T_j and the product of f with its line.
// T_j cannot stay in registers for eight pairs.  The Miller loop touches the slots 0 (f), 7 (C12_R1 / C12_B), 10 (C12_X), 11 (C12_I / C12_R2) and 12 (C12_R3); the
// eight others (1 .. 6, 8, 9) hold values of the final exponentiation and are dead until it starts.  A slot is 12 Fp per item, exactly the 12 Fp of a pair in the
// workspace map: lane (c, h) of the item keeps Fp number 2 c + h of P (2) | Q (4) | T (6), so Q is coefficients 1, 2 of the slot and T coefficients 3, 4, 5.
// Pair j lives in slot c12_pair_slot(j); the image stays at 13 slots.  A G2 step reads P, Q and T whole before the lanes of T write their halves back.
__device__ __forceinline__ int c12_pair_slot(int j) { return j < 6 ? j + 1 : j + 2; }
static_assert(VP_MAX_PAIRS == 8 && VP_PAIR_ELEMS == 12, "one LDS slot per pair: eight slots are free during the Miller loop, a slot is twelve Fp per item");
__global__ void __launch_bounds__(64)
k_coop12_miller_pairs(int32_t* ws, uint32_t n, uint8_t* status, const uint8_t* __restrict__ kinds, int n_pairs, const int32_t* __restrict__ target) {
  C12_PROLOGUE();
  int np = __builtin_amdgcn_readfirstlane(n_pairs);
  np = np < 1 ? 1 : (np > VP_MAX_PAIRS ? VP_MAX_PAIRS : np);
  const int F = C12_SLOT(VE_F);
  const uint32_t l12 = 2 * c + h;
  const uint32_t ident = (uint32_t)ws[(size_t)VP_IDENT * BN_NL * n + pc];      // digit 0 of VP_IDENT: the item's identity bits
  co.put(F, l12 == 0 ? fp_one() : fp_zero());
  for (int j = 0; j < np; j++) {   // P | Q as the loader left them (vp_p(j) .. + 5), T = (Q, 1)
    const Fp v = c12_ws_ld(ws, n, pc, l12 < 6 ? vp_p(j) + (int)l12 : l12 < 10 ? vp_q(j) + (int)l12 - 6 : vp_p(j));
    co.put(c12_pair_slot(j), l12 == 10 ? fp_one() : l12 == 11 ? fp_zero() : v);
  }
  for (int s = 0; s < BN_ATE_STEPS; s++) {
    const int kind = __builtin_amdgcn_readfirstlane((int)kinds[s]);
    if (kind == 0 && s != 0) c12_sqr(co, F);
    for (int j = 0; j < np; j++) {
      const int sl = c12_pair_slot(j);
      const Fp xa = co.at(sl, co.g0), ya = co.at(sl, co.g0 + 1);
      G2Proj t; t.x = co.coef(sl, 3); t.y = co.coef(sl, 4); t.z = co.coef(sl, 5);
      C12Line ln;
      if (kind == 0) {
        c12_g2_double_var(co, t, xa, ya, ln);
      } else {
        G2Aff q; q.x = co.coef(sl, 1); q.y = co.coef(sl, 2);
        G2Aff b = q;
        if (kind == 2) b = g2_neg(q);
        else if (kind == 3) b = g2_psi_affine(q);
        else if (kind == 4) b = g2_neg(g2_psi2_affine(q));
        c12_g2_add_var(co, t, b.x, b.y, xa, ya, ln);
      }
      if (c >= 3) { const Fp2 nt = fp2_select(c == 3, t.x, fp2_select(c == 4, t.y, t.z)); co.put(sl, fp_select(h != 0, nt.c1, nt.c0)); }
      // a pair with an identity on either side contributes 1; its G2 steps above still ran: the r-torsion test of a finite Q_j beside the identity of G1 needs T_j
      c12_mul_line_fp2(co, F, c12_halves(ln.d0, h), c12_halves(ln.d3, h), c12_halves(ln.d4, h), vp_skips(ident, j));
    }
  }
  // the r-torsion test of every finite Q_j from T_j (vm_g2_ate_check; c12_g16_verdict), every lane for itself, before the final exponentiation takes the slots
  bool in_g2 = true;
  for (int j = 0; j < np; j++) {
    const int sl = c12_pair_slot(j);
    const Fp2 qx = co.coef(sl, 1), qy = co.coef(sl, 2), X = co.coef(sl, 3), Y = co.coef(sl, 4), Z = co.coef(sl, 5);
    const Fp2 sx = fp2_mul(fp2_conj(qx), frob_coeff(3, 2)), sy = fp2_neg(fp2_mul(fp2_conj(qy), frob_coeff(3, 3)));
    const bool ok = !fp2_is_zero(Z) & fp2_eq(X, fp2_mul(sx, Z)) & fp2_eq(Y, fp2_mul(sy, Z));
    in_g2 &= ok | !vp_q_finite(ident, j);
  }
  Coop12Ops ops{co};
  vm_final_exp_program(ops);
  const bool writer = pending && c == 0 && h == 0;
  if (target) {   // the verdict in the launch
    const bool acc = c12_eq_const(co, C12_SLOT(VE_S0), target, pl);
    if (writer) status[p] = !in_g2 ? BN254_ST_NOT_IN_SUBGROUP : acc ? BN254_ST_ACCEPT : BN254_ST_REJECT;
    return;
  }
  // the GT value to VE_S0 for the tails of the lane form (k_pairing_store, k_g16_compare), which pass over an item that is no longer pending
  if (writer && !in_g2) status[p] = BN254_ST_NOT_IN_SUBGROUP;
  c12_store_f12(co, ws, n, p, C12_SLOT(VE_S0), VE_S0, pending && in_g2);
}

}  // namespace bn254

using namespace bn254;
// device copy of the step-kind table (88 bytes), created on first use per device
static const uint8_t* c12_kinds_dev() {
  static uint8_t* dev[64] = {nullptr};
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  int d = 0; (void)hipGetDevice(&d);
  if (d < 0 || d >= 64) return nullptr;
  if (!dev[d]) {
    if (hipMalloc((void**)&dev[d], BN_ATE_STEPS) != hipSuccess) return nullptr;
    (void)hipMemcpy(dev[d], miller_step_table().kind, BN_ATE_STEPS, hipMemcpyHostToDevice);
  }
  return dev[d];
}
hipError_t bn254_coop12_prepare() { return c12_kinds_dev() ? hipSuccess : hipErrorOutOfMemory; }
// one wavefront per five proofs with its LDS image; every kernel starts (ws, n, status), a Miller kernel takes the step-kind table next
template <bool KINDS, class Kernel, class... Args>
static hipError_t c12_launch(Kernel kernel, int32_t* ws, uint8_t* status, size_t n, hipStream_t s, Args... args) {
  const size_t lds = (size_t)C12_WAVE_DWORDS * 4;
  const dim3 grid((unsigned)((n + C12_PER_WAVE - 1) / C12_PER_WAVE));
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if constexpr (KINDS) {
    const uint8_t* kinds = c12_kinds_dev();
    if (!kinds) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(kernel, grid, dim3(64), lds, s, ws, (uint32_t)n, status, kinds, args...);
  } else hipLaunchKernelGGL(kernel, grid, dim3(64), lds, s, ws, (uint32_t)n, status, args...);
  return hipGetLastError();
}
hipError_t bn254_coop12_final_exp(int32_t* ws, uint8_t* status, size_t n, hipStream_t s) { return c12_launch<false>(k_coop12_final_exp, ws, status, n, s); }
hipError_t bn254_coop12_miller_fixed(int32_t* ws, uint8_t* status, size_t n, int n_pairs, const int32_t* tab0, const int32_t* tab1, const int32_t* target, int reject_code,
                                     hipStream_t s) {
  return c12_launch<true>(k_coop12_miller_fixed, ws, status, n, s, n_pairs, tab0, tab1, target, reject_code);
}
hipError_t bn254_coop12_miller_g16(int32_t* ws, uint8_t* status, size_t n, const int32_t* tab0, const int32_t* tab1, const uint8_t* inputs, int n_public,
                                   int inputs_match_key, const int32_t* msm_tab, const int32_t* k0, int l_from_ws, const int32_t* target, hipStream_t s) {
  return c12_launch<true>(k_coop12_miller_g16, ws, status, n, s, tab0, tab1, inputs, n_public, inputs_match_key, msm_tab, k0, l_from_ws, target);
}
hipError_t bn254_coop12_miller_g16_keys(int32_t* ws, uint8_t* status, size_t n, const uint32_t* key_index, const bn254::G16KeyDesc* desc, uint32_t n_keys, const uint8_t* inputs,
                                        size_t input_stride, int strict_scalars, hipStream_t s) {
  return c12_launch<true>(k_coop12_miller_g16_keys, ws, status, n, s, key_index, desc, n_keys, inputs, input_stride, strict_scalars);
}
hipError_t bn254_coop12_miller_fixed_keys(int32_t* ws, uint8_t* status, size_t n, const uint32_t* key_words, uint32_t key_shift, const bn254::PlonkKeyDesc* desc, uint32_t n_keys,
                                          const int32_t* target, int reject_code, hipStream_t s) {
  if (n == 0 || n_keys == 0 || key_shift > 31) return hipErrorInvalidValue;
  return c12_launch<true>(k_coop12_miller_fixed_keys, ws, status, n, s, key_words, key_shift, desc, n_keys, target, reject_code);
}
hipError_t bn254_coop12_miller_pairs(int32_t* ws, uint8_t* status, size_t n, int n_pairs, const int32_t* target, hipStream_t s) {
  if (n == 0 || n > (size_t)COOP12_MAX_PROOFS || n_pairs < 1 || n_pairs > VP_MAX_PAIRS) return hipErrorInvalidValue;
  return c12_launch<true>(k_coop12_miller_pairs, ws, status, n, s, n_pairs, target);
}
// probe: op 0 mul 1 mul by conj(b) 2 conj(a) * b 3 sqr 4 cyclo_sqr_n (arg squarings) 5 frob (j = arg) 6 inv 7 conj 8 mul_line_fp 9 mul_line_fp with keep
// 10 mul_line_fp2 11 k_coop12_final_exp 12 c12_eq_const against target
hipError_t bn254_coop12_dbg_op(int32_t* ws, uint8_t* status, size_t n, int op, int arg, const int32_t* target, hipStream_t s) {
  if (op == 11) return bn254_coop12_final_exp(ws, status, n, s);
  return c12_launch<false>(k_coop12_dbg_op, ws, status, n, s, op, arg, target);
}
