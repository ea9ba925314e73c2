// bn254_k_g16_load.hip -- what brings a Groth16 batch into the workspace, and the record plumbing around the raw pipeline:
//   k_g16_classify, k_g16_compact_write   compaction of a lane launch (bn254_g16_plan.h::g16_compacts)
//   k_g16_prepare                         parse and checks of A, B, C (bn254_g16_loader.h), L = K0 + sum x_i K_i by fixed-base 13-bit windows
//   k_g16_check_scalars                   BN254_FLAG_STRICT_SCALARS
//   k_g16_msm_partial, k_g16_comb_digits, k_g16_msm_partial_comb, k_g16_msm_reduce, k_g16_msm_reduce8     L of a key with many public inputs
//   k_gather_rows, k_scatter_status       the rows of the RLC mode's exact second pass
//   k_g16_decompress, k_g16_status_merge  BN254_FLAG_COMPRESSED_PROOFS
//   k_sp1_public_inputs                   SP1 public inputs, hashed from the public values
// The loader and MSM kernels are launched where a batch is enqueued -- bn254_launch_g16 (bn254_kernels.hip), bn254_launch_g16_rlc (bn254_k_rlc.hip), the probes
// (bn254_k_probe.hip) -- through their declarations in bn254_launch_ops.h; the launchers of the record utilities are at the end of this file.
#include <hip/hip_runtime.h>
#include "bn254_launch_ops.h"
#include "bn254_g16_loader.h"
#include "bn254_g16_plan.h"
#include "bn254_codec.h"
#include "bn254_sha256.h"

namespace bn254 {
// Compiled twice (Makefile): the first object holds everything but the body of k_g16_decompress; the second (-DBN_PLAIN_HALF -DBN_NO_CARRY_RIDE) holds only that kernel,
// which keeps the reassociated carry chains: with the carry ride it spills more (profiles/carry_chain_resources.txt).
#ifndef BN_PLAIN_HALF

// ---- compaction (bn254_g16_plan.h::g16_compacts): classify, then count -> scan -> write ------------------------------------------------------------------------------
// k_g16_classify, one proof per lane: the loader checks whose outcome is FINAL -- the range and curve checks of A and B, through the helpers and in the order of
// k_g16_prepare; the checks of C are deferred there (the r-torsion test of B ranks ahead of them) and do not run here.  status[i], the CALLER's byte, becomes the
// final status of a decided proof and BN254_ST_PENDING otherwise (so the buffer never keeps a byte of an earlier batch); block_count[b] = pending proofs of block b.
__global__ void __launch_bounds__(256, 2)
k_g16_classify(const uint8_t* __restrict__ proofs, size_t stride, uint32_t n, uint8_t* __restrict__ status, uint32_t* __restrict__ block_count) {
  __shared__ uint32_t lds[4 * 64 * PREP_LDS_ROW];
  __shared__ uint32_t wave_pending[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t first = blockIdx.x * 256u + (uint32_t)wave * 64u;
  uint32_t* wl = lds + wave * 64 * PREP_LDS_ROW;
  const uint32_t i = first + lane;
  const bool live = i < n;
  g16_stage_records(wl, proofs, stride, n, lane, i);
  __syncthreads();
  G1Aff A; G2Aff B;
  int err = g16_parse_a(wl + lane * PREP_LDS_ROW, A);
  err = g16_parse_b(wl + lane * PREP_LDS_ROW, B, err);
  if (live) status[i] = err ? (uint8_t)err : (uint8_t)BN254_ST_PENDING;
  const uint64_t pend = __builtin_amdgcn_ballot_w64(live && err == 0);
  if (lane == 0) wave_pending[wave] = (uint32_t)__builtin_popcountll(pend);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = wave_pending[0] + wave_pending[1] + wave_pending[2] + wave_pending[3];
}
// k_g16_compact_write, the grid of k_g16_classify: every block scans the (at most 3072) block counts for itself -- the pending proofs before it and in the whole
// launch, n' -- ranks its own pending proofs in order, and writes slot_proof[j] = proof of slot j, slot_status[j] = PENDING for j < n'; the lane of slot j >= n'
// writes slot_status[j] = 0 (no later kernel works on it) and slot_proof[j] = no proof.  Order-preserving and the same on every run: no slot is taken by an atomic.
__global__ void __launch_bounds__(256)
k_g16_compact_write(const uint8_t* __restrict__ status, uint32_t n, const uint32_t* __restrict__ block_count, uint32_t* __restrict__ slot_proof, uint8_t* __restrict__ slot_status) {
  __shared__ uint32_t s_before[G16_COMPACT_BLOCK], s_total[G16_COMPACT_BLOCK], wave_pending[4];
  const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
  uint32_t before, total;
  g16_compact_partial(block_count, gridDim.x, blockIdx.x, t, &before, &total);
  s_before[t] = before; s_total[t] = total;
  const uint32_t i = blockIdx.x * 256u + t;
  const bool pend = i < n && status[i] == BN254_ST_PENDING;
  const uint64_t mask = __builtin_amdgcn_ballot_w64(pend);
  if (lane == 0) wave_pending[wave] = (uint32_t)__builtin_popcountll(mask);
  __syncthreads();
  for (uint32_t d = G16_COMPACT_BLOCK / 2; d > 0; d >>= 1) {
    if (t < d) { s_before[t] += s_before[t + d]; s_total[t] += s_total[t + d]; }
    __syncthreads();
  }
  const uint32_t n_pending = s_total[0];
  uint32_t j = s_before[0] + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < wave; k++) j += wave_pending[k];
  if (pend && j < n) { slot_proof[j] = i; slot_status[j] = BN254_ST_PENDING; }
  if (i < n && i >= n_pending) { slot_proof[i] = G16_COMPACT_NO_PROOF; slot_status[i] = 0; }
}

// slot_proof != nullptr, a launch that compacts: the kernel works on SLOT i -- the record and the inputs of proof slot_proof[i], workspace column i, and its status
// byte goes to slot_status[i], which k_g16_compact_write has set (PENDING below n', 0 from there on: such a wavefront has nothing to do).  The staging is then a
// gather of whole 256-byte records, still one segment per load instruction.
__global__ void __launch_bounds__(256, 2)
k_g16_prepare(const uint8_t* __restrict__ proofs, size_t stride, const uint8_t* __restrict__ inputs, int n_public, uint32_t n,
              int32_t* ws, uint8_t* __restrict__ status, const int32_t* __restrict__ msm_tab, const int32_t* __restrict__ k0,
              int inputs_match_key, int wide_msm, const uint32_t* __restrict__ slot_proof, uint8_t* __restrict__ slot_status) {
  __shared__ uint32_t lds[4 * 64 * PREP_LDS_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t first = blockIdx.x * 256u + (uint32_t)wave * 64u;
  uint32_t* wl = lds + wave * 64 * PREP_LDS_ROW;
  uint32_t pi = first + (uint32_t)lane;     // the proof of this lane
  bool wave_live = true;
  if (slot_proof) {
    const bool slot_live = pi < n && (slot_status[pi] & BN254_ST_PENDING) != 0;
    pi = slot_live ? slot_proof[pi] : G16_COMPACT_NO_PROOF;
    wave_live = __builtin_amdgcn_ballot_w64(slot_live) != 0;
  }
  if (wave_live) g16_stage_records(wl, proofs, stride, n, lane, pi);
  __syncthreads();
  if (!wave_live) return;
  uint8_t* const st_out = slot_proof ? slot_status : status;
  const uint32_t i = first + lane;
  const bool live = pi < n;
  const uint32_t ii = live ? pi : n - 1;
  // dead lanes get an out-of-range lane offset: the descriptor's bounds check drops their stores
  DevWs w(ws, n, live ? i : DEAD_LANE);
  const uint32_t* my = wl + lane * PREP_LDS_ROW;

  // ---- A, then B: the first error in the reference's order -- A, then B (member, curve), B subgroup (the Miller loop's tail), then C
  G1Aff A;
  int err = g16_parse_a(my, A);
  w.st(VE_AX, A.x); w.st(VE_AY, A.y);
  G2Aff B;
  err = g16_parse_b(my, B, err);
  vst2(w, VE_B, B.x); vst2(w, VE_B + 2, B.y);

  G1Aff C;
  const int err_c = g16_parse_c(my, C);
  w.st(VE_CX, C.x); w.st(VE_CY, C.y);

  // ---- L = K0 + sum_i x_i K_i, x_i taken as raw 256-bit integers (no range check, as bn::Fr::from_slice)
  if (wide_msm) {
    // many public inputs: L comes from k_g16_msm_partial / k_g16_msm_reduce (they also set the identity flag)
    if (live) st_out[i] = err ? (uint8_t)err : (uint8_t)(BN254_ST_PENDING | err_c);
    return;
  }
  G1Aff K0; K0.x = uni_ld(k0); K0.y = uni_ld(k0 + BN_NL);
  G1Proj L = g1_from_affine(K0);
  if (inputs_match_key) {
    for (int s = 0; s < n_public; s++) {
      const uint8_t* sp = inputs + ((size_t)ii * (size_t)n_public + s) * 32;
      uint32_t sw[8];
      if ((((uintptr_t)inputs) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) sw[k] = ((const uint32_t*)sp)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) sw[k] = (uint32_t)sp[4 * k] | (uint32_t)sp[4 * k + 1] << 8 | (uint32_t)sp[4 * k + 2] << 16 | (uint32_t)sp[4 * k + 3] << 24;
      }
      // sw[] holds the big-endian scalar as it lies in memory; kw[i] = bits 32 i .. 32 i + 31 of its value.  Window wi (MSM_FW_BITS = 13 bits, weight 2^(13 wi): bn254_fw.h --
      // 20 table additions per input where the byte windows of rounds 1-4 made 32) is consumed from the low end of kw[0] and the 256-bit array is shifted down by 13 each
      // time: no dynamic register indexing.  The 80-byte table entry of window wi + 1 (18 digits + 2 pad, 16-byte aligned: five 16-byte loads per lane) is in flight
      // while the addition of window wi runs.
      uint32_t kw[8];
#pragma unroll
      for (int k = 0; k < 8; k++) kw[k] = __builtin_bswap32(sw[7 - k]);
      auto next_digit = [&]() -> uint32_t {
        const uint32_t dg = kw[0] & MSM_FW_ENTRIES;
#pragma unroll
        for (int k = 0; k < 7; k++) kw[k] = (kw[k] >> MSM_FW_BITS) | (kw[k + 1] << (32 - MSM_FW_BITS));
        kw[7] >>= MSM_FW_BITS;
        return dg;
      };
      uint32_t dig = next_digit();
      G1Aff q = msm_entry(msm_tab, (size_t)(s * MSM_FW_WINDOWS) * MSM_FW_ENTRIES + (dig ? dig - 1 : 0));
      for (int j = 0; j < MSM_FW_WINDOWS; j++) {
        uint32_t dn = 0; G1Aff qn = q;
        if (j + 1 < MSM_FW_WINDOWS) { dn = next_digit(); qn = msm_entry(msm_tab, (size_t)(s * MSM_FW_WINDOWS + j + 1) * MSM_FW_ENTRIES + (dn ? dn - 1 : 0)); }
        if (dig != 0) L = g1_add_mixed(L, q);
        dig = dn; q = qn;
      }
    }
  }
  // to affine (one inversion per proof); the identity -- unreachable without a discrete-log relation between the K_i -- is kept
  // as (0, 1) plus a flag bit, and the Miller kernel makes its line value 1 (bn::pairing_batch skips such pairs)
  bool l_inf = g1_is_identity(L);
  G1Aff La = g1_to_affine(L);
  La.y = fp_select(l_inf, fp_one(), La.y);
  w.st(VE_LX, La.x); w.st(VE_LY, La.y);
  if (live) st_out[i] = err ? (uint8_t)err : (uint8_t)(BN254_ST_PENDING | (l_inf ? BN254_ST_LINF : 0) | err_c);
}

// BN254_FLAG_STRICT_SCALARS: a public input >= r makes the proof's status NOT_MEMBER, ahead of every other outcome (the
// reference's bn::Fr::from_slice does not range-check; this is the opt-in stricter policy).  Runs right after
// k_g16_prepare, so that such proofs are no longer pending for the rest of the pipeline.
__global__ void __launch_bounds__(256, 2)
k_g16_check_scalars(const uint8_t* __restrict__ inputs, int n_public, uint32_t n, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  bool bad = false;
  for (int s = 0; s < n_public; s++) {
    const uint8_t* sp = inputs + ((size_t)i * (size_t)n_public + s) * 32;
    uint32_t w[8];
    words_from_be(w, sp);
    bad |= words_ge(w, BN_R_WORDS);
  }
  if (bad) status[i] = BN254_ST_NOT_MEMBER;
}

// =====================================================================================================================
// public-input MSM for keys with many inputs (BASELINE config 5: 1024): the inputs of one proof are spread over `chunks` lanes
// =====================================================================================================================
// lane g = c * n + i: chunk c of proof i sums inputs [c * per, min((c+1) * per, n_public)); partial sums (projective, 27 dwords)
// go to part[(c * 27 + k) * n + i]: every access of a wave is contiguous over proofs.
__global__ void __launch_bounds__(256, 2)
k_g16_msm_partial(const uint8_t* __restrict__ inputs, int n_public, uint32_t n, int per, int chunks, const uint8_t* __restrict__ status,
                  const int32_t* __restrict__ msm_tab, int32_t* __restrict__ part) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n * (uint32_t)chunks) return;
  const uint32_t c = g / n, i = g - c * n;
  G1Proj acc = g1_identity();
  if (status[i] & BN254_ST_PENDING) {
    const int s_end = (int)min((uint32_t)n_public, (c + 1) * (uint32_t)per);
    for (int s = (int)(c * per); s < s_end; s++) {
      const uint8_t* sp = inputs + ((size_t)i * (size_t)n_public + s) * 32;
      uint32_t sw[8];
      if ((((uintptr_t)inputs) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) sw[k] = ((const uint32_t*)sp)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) sw[k] = (uint32_t)sp[4 * k] | (uint32_t)sp[4 * k + 1] << 8 | (uint32_t)sp[4 * k + 2] << 16 | (uint32_t)sp[4 * k + 3] << 24;
      }
      for (int j = 0; j < 32; j++) {  // byte j of the big-endian scalar = window 31 - j (as in k_g16_prepare)
        const int wi = 31 - j;
        uint32_t dig = sw[0] & 0xff;
#pragma unroll
        for (int k = 0; k < 7; k++) sw[k] = (sw[k] >> 8) | (sw[k + 1] << 24);
        sw[7] >>= 8;
        if (dig != 0) acc = g1_add_mixed(acc, msm_entry(msm_tab, (size_t)(s * 32 + wi) * 255 + (dig - 1)));
      }
    }
  }
  int32_t* o = part + (size_t)c * 27 * n + i;
#pragma unroll
  for (int l = 0; l < BN_NL; l++) { o[(size_t)l * n] = acc.x.v[l]; o[(size_t)(9 + l) * n] = acc.y.v[l]; o[(size_t)(18 + l) * n] = acc.z.v[l]; }
}
// The same sum from COMB tables (bn254_host.hpp::build_comb_table; keys prepared with msm_comb): the lane walks the G16_COMB_COLS = 20 columns
// from the top, doubling its accumulator once per column and adding, for each of its inputs, the entry selected by bits c, c + 20, ..., c + 240 of
// the scalar (G16_COMB_TEETH = 13 bits): 20 additions per input and 20 doublings per lane instead of 32 additions per input.
// k_g16_comb_digits first turns every scalar (big-endian bytes: bit b of the integer is bit b % 8 of byte 31 - b / 8) into its 20 column digits,
// stored transposed -- digits[(col * n_public + s) * n + i] -- so that the lanes of a wavefront (consecutive proofs) read consecutive u16.
__global__ void __launch_bounds__(256)
k_g16_comb_digits(const uint8_t* __restrict__ inputs, int n_public, uint32_t n, uint16_t* __restrict__ digits) {
  const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= (size_t)n * (size_t)n_public) return;
  const uint32_t s = (uint32_t)(g / n), i = (uint32_t)(g - (size_t)s * n);
  const uint8_t* sp = inputs + ((size_t)i * (size_t)n_public + s) * 32;
  uint32_t w[8];   // w[k]: bits 32 k .. 32 k + 31 of the integer
#pragma unroll
  for (int k = 0; k < 8; k++) { const uint8_t* q = sp + 28 - 4 * k; w[k] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3]; }
  for (int col = 0; col < G16_COMB_COLS; col++) {
    const uint32_t idx = g16_comb_digit(w, col);
    digits[((size_t)col * (size_t)n_public + s) * n + i] = (uint16_t)idx;
  }
}
__global__ void __launch_bounds__(256, 2)
k_g16_msm_partial_comb(const uint16_t* __restrict__ digits, int n_public, uint32_t n, int per, int chunks, const uint8_t* __restrict__ status,
                       const int32_t* __restrict__ msm_tab, int32_t* __restrict__ part) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n * (uint32_t)chunks) return;
  const uint32_t c = g / n, i = g - c * n;
  G1Proj acc = g1_identity();
  if (status[i] & BN254_ST_PENDING) {
    const int s_begin = (int)(c * per), s_end = (int)min((uint32_t)n_public, (c + 1) * (uint32_t)per);
    // Software pipeline (round 4): the table entry of addition k + 1 (a random 80-byte read of a 671 MB table) and the digit of addition k + 2 are in flight while
    // addition k computes.  Without it every addition waited for its own digit, then for its own entry, with two wavefronts per SIMD to hide that behind
    // (VALU-active 0.37, profiles/r02_cfg5_pmc_summary.csv).  (col, s) walks the columns from the top, the chunk's inputs inside a column.
    auto digit_at = [&](int col, int s) -> uint32_t { return digits[((size_t)col * (size_t)n_public + (size_t)s) * n + i]; };
    auto entry_at = [&](int s, uint32_t idx) -> G1Aff { return msm_entry(msm_tab, ((size_t)s << G16_COMB_TEETH) + idx); };   // idx 0: a valid (unused) slot of the table
    auto advance = [&](int& col, int& s) { if (++s == s_end) { s = s_begin; col--; } };
    if (s_begin < s_end) {
      int col1 = G16_COMB_COLS - 1, s1 = s_begin;            // position of addition k + 1 while addition k runs
      uint32_t d_cur = digit_at(col1, s1);
      G1Aff e_cur = entry_at(s1, d_cur);
      int col0 = col1, s0 = s1;
      advance(col1, s1);
      uint32_t d_nxt = col1 >= 0 ? digit_at(col1, s1) : 0u;
      int col2 = col1, s2 = s1;                               // position of addition k + 2
      if (col2 >= 0) advance(col2, s2);
      while (col0 >= 0) {
        G1Aff e_nxt = e_cur;
        uint32_t d_nn = 0u;
        if (col1 >= 0) e_nxt = entry_at(s1, d_nxt);
        if (col2 >= 0) d_nn = digit_at(col2, s2);
        if (s0 == s_begin && col0 != G16_COMB_COLS - 1) acc = g1_dbl(acc);
        if (d_cur != 0) acc = g1_add_mixed(acc, e_cur);
        col0 = col1; s0 = s1; d_cur = d_nxt; e_cur = e_nxt;
        col1 = col2; s1 = s2; d_nxt = d_nn;
        if (col2 >= 0) advance(col2, s2);
      }
    }
  }
  int32_t* o = part + (size_t)c * 27 * n + i;
#pragma unroll
  for (int l = 0; l < BN_NL; l++) { o[(size_t)l * n] = acc.x.v[l]; o[(size_t)(9 + l) * n] = acc.y.v[l]; o[(size_t)(18 + l) * n] = acc.z.v[l]; }
}
// L = K0 + sum of the chunk sums (complete projective additions), to affine, identity flag into the status byte
__global__ void __launch_bounds__(256, 2)
k_g16_msm_reduce(const int32_t* __restrict__ part, int chunks, uint32_t n, int32_t* ws, uint8_t* __restrict__ status, const int32_t* __restrict__ k0) {
  VM_KERNEL_PROLOGUE();
  const uint32_t ii = i < n ? i : n - 1;
  G1Aff K0; K0.x = uni_ld(k0); K0.y = uni_ld(k0 + BN_NL);
  G1Proj L = g1_from_affine(K0);
  for (int c = 0; c < chunks; c++) {
    const int32_t* o = part + (size_t)c * 27 * n + ii;
    G1Proj q;
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { q.x.v[l] = o[(size_t)l * n]; q.y.v[l] = o[(size_t)(9 + l) * n]; q.z.v[l] = o[(size_t)(18 + l) * n]; }
    BN_SETB(q.x, 3.0, 0.5); BN_SETB(q.y, 3.0, 0.5); BN_SETB(q.z, 3.0, 0.5);
    L = g1_add(L, q);
  }
  bool l_inf = g1_is_identity(L);
  G1Aff La = g1_to_affine(L);
  La.y = fp_select(l_inf, fp_one(), La.y);
  w.st(VE_LX, La.x); w.st(VE_LY, La.y);
  if (i < n && (st & BN254_ST_PENDING) && l_inf) status[i] = st | BN254_ST_LINF;
}

// The same with EIGHT lanes per proof (small batches, where the launch lasts as long as one lane's chain of `chunks` additions): lane `sub` adds the
// chunk sums sub, sub + 8, ..., the eight partial sums meet in LDS, lane 0 adds them to K0 and finishes: chunks / 8 + 8 additions in a row
// instead of chunks.  256 threads = 32 proofs.
__global__ void __launch_bounds__(256, 2)
k_g16_msm_reduce8(const int32_t* __restrict__ part, int chunks, uint32_t n, int32_t* ws, uint8_t* __restrict__ status, const int32_t* __restrict__ k0) {
  __shared__ int32_t sums[32 * 8 * 27];
  const uint32_t p = blockIdx.x * 32u + (threadIdx.x >> 3), sub = threadIdx.x & 7u;
  const uint32_t pp = p < n ? p : n - 1;
  G1Proj L = g1_identity();
  for (int c = (int)sub; c < chunks; c += 8) {
    const int32_t* o = part + (size_t)c * 27 * n + pp;
    G1Proj q;
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { q.x.v[l] = o[(size_t)l * n]; q.y.v[l] = o[(size_t)(9 + l) * n]; q.z.v[l] = o[(size_t)(18 + l) * n]; }
    BN_SETB(q.x, 3.0, 0.5); BN_SETB(q.y, 3.0, 0.5); BN_SETB(q.z, 3.0, 0.5);
    L = g1_add(L, q);
  }
  {
    int32_t* o = sums + threadIdx.x * 27;
    const Fp x = fp_reduce(L.x), y = fp_reduce(L.y), z = fp_reduce(L.z);
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { o[l] = x.v[l]; o[9 + l] = y.v[l]; o[18 + l] = z.v[l]; }
  }
  __syncthreads();
  const bool lead = sub == 0 && p < n;
  const uint8_t st = status[pp];
  G1Aff K0; K0.x = uni_ld(k0); K0.y = uni_ld(k0 + BN_NL);
  G1Proj T = g1_from_affine(K0);
  for (int j = 0; j < 8; j++) {       // every lane runs the tail (no divergence); only the leading lane's result is stored
    const int32_t* o = sums + ((threadIdx.x & ~7u) + j) * 27;
    G1Proj q;
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { q.x.v[l] = o[l]; q.y.v[l] = o[9 + l]; q.z.v[l] = o[18 + l]; }
    BN_SETB(q.x, 1.01, 0.5); BN_SETB(q.y, 1.01, 0.5); BN_SETB(q.z, 1.01, 0.5);
    T = g1_add(T, q);
  }
  const bool l_inf = g1_is_identity(T);
  G1Aff La = g1_to_affine(T);
  La.y = fp_select(l_inf, fp_one(), La.y);
  DevWs w(ws, n, lead ? p : DEAD_LANE);
  w.st(VE_LX, La.x); w.st(VE_LY, La.y);
  if (lead && (st & BN254_ST_PENDING) && l_inf) status[p] = st | BN254_ST_LINF;
}

// fallback plumbing: rows idx[k] of a strided byte array -> packed rows; statuses back
__global__ void k_gather_rows(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t src_stride, uint32_t row_bytes, const uint32_t* __restrict__ idx, uint32_t m) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t per = row_bytes / 4;
  if (t >= (size_t)m * per) return;
  const uint32_t k = (uint32_t)(t / per), c = (uint32_t)(t % per);
  const uint8_t* p = src + (size_t)idx[k] * src_stride + 4 * (size_t)c;
  uint32_t v;
  if ((((uintptr_t)src) | src_stride) & 3) v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
  else v = *(const uint32_t*)p;
  ((uint32_t*)dst)[t] = v;
}
__global__ void k_scatter_status(uint8_t* __restrict__ status, const uint8_t* __restrict__ fb_status, const uint32_t* __restrict__ idx, uint32_t m) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < m) status[idx[k]] = fb_status[k];
}
// BN254_FLAG_COMPRESSED_PROOFS: one compressed record per lane (bn254_codec.h::g16_decompress_record, the code bn254_dbg_g16_decompress runs on the
// host) -> the 256-byte raw record at raw + 256 i, and pre[i] = 1 if it did not decompress (its raw record is then all ones, which the loader answers with
// NOT_MEMBER; k_g16_status_merge turns the final status into MALFORMED).  About 1 900 field products per lane (two Fp roots, one Fp2 root): compute-bound,
// so the 128-byte record is simply loaded per lane -- four 16-byte loads when the records are 16-byte aligned (stride 128), bytes otherwise.
#endif
__global__ void __launch_bounds__(256, 2) k_g16_decompress(const uint8_t* __restrict__ src, size_t stride, uint32_t n, uint8_t* __restrict__ raw, uint8_t* __restrict__ pre)
#ifdef BN_PLAIN_HALF
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = src + (size_t)i * stride;
  uint32_t in[32], out[64];
  if (((((uintptr_t)src) | stride) & 15) == 0) {   // wave-uniform
#pragma unroll
    for (int k = 0; k < 8; k++) { const uint4 v = ((const uint4*)p)[k]; in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w; }
  } else {
#pragma unroll
    for (int k = 0; k < 32; k++) in[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
  }
  const bool ok = g16_decompress_record(in, out);
  uint4* q = (uint4*)(raw + (size_t)i * 256);
#pragma unroll
  for (int k = 0; k < 16; k++) q[k] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
  pre[i] = ok ? 0 : 1;
}
#else
;
#endif
#ifndef BN_PLAIN_HALF
// after the raw pipeline over the decompressed records: a record that did not decompress is MALFORMED, whatever the loader said about its all-ones stand-in
__global__ void __launch_bounds__(256) k_g16_status_merge(uint8_t* __restrict__ status, const uint8_t* __restrict__ pre, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n && pre[i]) status[i] = BN254_ST_MALFORMED;
}
// SP1 public inputs (bn254_sha256.h): one proof per lane.  Lane i hashes bytes [off[i] - pv_base, off[i+1] - pv_base) of pv (pv_bytes long) and writes the 64-byte
// row vkey_hash_i | digest_i to rows + 64 i, and pre[i] = 1 if the range is not inside the buffer (the row then carries the digest of the empty string).  The
// block loop is wavefront-uniform: it runs to the longest message of the wavefront (a ballot of "this lane has a block left" ends it), and a lane that has no
// block left computes and discards it -- no lane leaves early, so the 64 rounds run once per block for the whole wavefront.  About 1 850 VALU instructions
// per block; the loads are aligned dwords.  No LDS, no scratch.
__global__ void __launch_bounds__(256) k_sp1_public_inputs(const uint8_t* __restrict__ vkh, size_t vkh_stride, const uint8_t* __restrict__ pv, uint64_t pv_bytes,
                                                           uint64_t pv_base, const uint64_t* __restrict__ off, uint32_t n, uint8_t* __restrict__ rows,
                                                           uint8_t* __restrict__ pre) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool lane = i < n;
  uint64_t start = 0, len = 0;
  bool ok = false;
  if (lane) ok = sp1_range(off[i], off[i + 1], pv_base, pv_bytes, &start, &len);
  const uint64_t nb = lane ? sha256_blocks(len) : 0;
  uint32_t h[8];
  sha256_init(h);
  for (uint64_t b = 0; __ballot(b < nb) != 0; b++) sp1_sha256_block(h, pv, pv_bytes, start, len, b);
  if (!lane) return;
  uint32_t v[8], dg[8];
  sp1_load_vkey_hash(vkh + (size_t)i * vkh_stride, v);
  sp1_digest_words(h, dg);
  uint4* q = (uint4*)(rows + (size_t)i * 64);
  q[0] = make_uint4(v[0], v[1], v[2], v[3]); q[1] = make_uint4(v[4], v[5], v[6], v[7]);
  q[2] = make_uint4(dg[0], dg[1], dg[2], dg[3]); q[3] = make_uint4(dg[4], dg[5], dg[6], dg[7]);
  pre[i] = ok ? 0 : 1;
}

#endif
}  // namespace bn254
#ifndef BN_PLAIN_HALF

// ---- launch wrappers (C++ linkage, declared in bn254_kernels.h) -----------------------------------------------------------
using namespace bn254;
hipError_t bn254_launch_gather_rows(uint8_t* dst, const uint8_t* src, size_t src_stride, uint32_t row_bytes, const uint32_t* idx, uint32_t m, hipStream_t s) {
  const size_t threads = (size_t)m * (row_bytes / 4);
  if (threads) hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, dst, src, src_stride, row_bytes, idx, m);
  return hipGetLastError();
}
hipError_t bn254_launch_scatter_status(uint8_t* status, const uint8_t* fb_status, const uint32_t* idx, uint32_t m, hipStream_t s) {
  if (m) hipLaunchKernelGGL(k_scatter_status, dim3(grid_for(m)), dim3(256), 0, s, status, fb_status, idx, m);
  return hipGetLastError();
}
hipError_t bn254_launch_g16_decompress(const uint8_t* src, size_t stride, uint32_t n, uint8_t* raw, uint8_t* pre, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_g16_decompress, dim3(grid_for(n)), dim3(256), 0, s, src, stride, n, raw, pre);
  return hipGetLastError();
}
hipError_t bn254_launch_g16_status_merge(uint8_t* status, const uint8_t* pre, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_g16_status_merge, dim3(grid_for(n)), dim3(256), 0, s, status, pre, n);
  return hipGetLastError();
}
hipError_t bn254_launch_sp1_public_inputs(const uint8_t* vkh, size_t vkh_stride, const uint8_t* pv, uint64_t pv_bytes, uint64_t pv_base, const uint64_t* off, uint32_t n,
                                          uint8_t* rows, uint8_t* pre, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_sp1_public_inputs, dim3(grid_for(n)), dim3(256), 0, s, vkh, vkh_stride, pv, pv_bytes, pv_base, off, n, rows, pre);
  return hipGetLastError();
}
#endif
