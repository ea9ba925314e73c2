// bn254_sha256.h -- SP1's public-input rule, compiled for the host AND the device: k_sp1_public_inputs and bn254_dbg_sp1_public_inputs(device = -1) run
// these same functions, and bn254_sp1_public_values_digest uses them too.
//
//   committed_values_digest = SHA-256(public_values) with the top three bits of byte 0 cleared
//   circuit inputs          = vkey_hash | committed_values_digest                        (two 32-byte big-endian words)
//
// SHA-256 is FIPS 180-4.  The message is read straight from the caller's values buffer as aligned dwords: one block of a lane is the 17 dwords around
// its 64 bytes, realigned with alignbyte and byte-swapped in registers; the padding byte and the 64-bit length are made in registers on the last one or
// two blocks.  Nothing is read outside [buf, buf + buf_bytes): a window that would cross either end is loaded dword by dword, and byte by byte where a
// dword itself crosses it.
//
// This is a second copy of the compression function: Sha256 in bn254_plonk.hpp (the PlonK transcripts) is left as it is, because the PlonK kernels are
// sensitive to what gets inlined around their hashes and their recorded per-kernel counts must not move.  The digest is handed on
// as byte-swapped dwords, never as field limbs, so the "digest -> 64-bit limbs -> multiply" pattern of the ROCm 7.2 miscompile does not arise here.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SHA_HD __host__ __device__ __forceinline__
#else
#define SHA_HD inline
#endif

namespace bn254 {

constexpr uint32_t SHA256_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
    0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
    0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

SHA_HD uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
// bytes s .. s + 3 of the little-endian 8-byte value hi:lo (s in 0..3): v_alignbyte_b32 on the device
SHA_HD uint32_t sha_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3)));
#endif
}

SHA_HD void sha256_init(uint32_t h[8]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au; h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}
// one compression: the 16-word schedule window and the 64 rounds fully unrolled (all indices are compile-time constants: registers only)
SHA_HD void sha256_compress(uint32_t h[8], const uint32_t win[16]) {
  uint32_t w[16];
#pragma unroll
  for (int t = 0; t < 16; t++) w[t] = win[t];
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; t++) {
    uint32_t wt;
    if (t < 16) wt = w[t];
    else {
      const uint32_t x = w[(t + 1) & 15], y = w[(t + 14) & 15];
      const uint32_t s0 = sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3), s1 = sha_rotr(y, 17) ^ sha_rotr(y, 19) ^ (y >> 10);
      wt = w[t & 15] = w[t & 15] + s0 + w[(t + 9) & 15] + s1;
    }
    const uint32_t t1 = hh + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) + SHA256_K[t] + wt;
    const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// blocks of a padded message of len bytes: len + 1 (0x80) + 8 (bit length) rounded up to 64
SHA_HD uint64_t sha256_blocks(uint64_t len) { return (len + 8) / 64 + 1; }

// The range of proof i: bytes [o0 - base, o1 - base) of a buffer of buf_bytes bytes (base: the offset the buffer's first byte has; 0 for the caller's own buffer).
// false (and an empty range) unless base <= o0 <= o1 and o1 - base <= buf_bytes.
SHA_HD bool sp1_range(uint64_t o0, uint64_t o1, uint64_t base, uint64_t buf_bytes, uint64_t* start, uint64_t* len) {
  const bool ok = o0 >= base && o1 >= o0 && o1 - base <= buf_bytes;
  *start = ok ? o0 - base : 0;
  *len = ok ? o1 - o0 : 0;
  return ok;
}

// the dword at byte address a (a multiple of 4) with only the bytes inside [lo, hi) read; the others are zero
SHA_HD uint32_t sp1_dword_guarded(uintptr_t a, uintptr_t lo, uintptr_t hi) {
  if (a >= lo && a + 4 <= hi) return *(const uint32_t*)a;
  uint32_t v = 0;
  for (int e = 0; e < 4; e++)
    if (a + e >= lo && a + e < hi) v |= (uint32_t)*(const uint8_t*)(a + e) << (8 * e);
  return v;
}

// Block `blk` of the message of len bytes at buf + start, compressed into h -- or h left as it is when the message has fewer blocks (a lane that is
// done while others of its wavefront are not: the block is computed and discarded, so the wavefront runs one path).  Message words past the end of
// the message are replaced by the padding; the bit length goes into words 14 and 15 of the last block.
SHA_HD void sp1_sha256_block(uint32_t h[8], const uint8_t* buf, uint64_t buf_bytes, uint64_t start, uint64_t len, uint64_t blk) {
  const uint64_t nb = sha256_blocks(len), pos = 64 * blk;
  uint32_t d[17];
#pragma unroll
  for (int k = 0; k < 17; k++) d[k] = 0;
  const uintptr_t lo = (uintptr_t)buf, hi = lo + buf_bytes;
  const uintptr_t addr = lo + start + pos, al = addr & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)(addr & 3);
  if (pos < len) {                               // a block that holds message bytes
    if (al >= lo && al + 68 <= hi) {             // the whole 17-dword window lies inside the buffer: plain aligned loads
      const uint32_t* q = (const uint32_t*)al;
#pragma unroll
      for (int k = 0; k < 17; k++) d[k] = q[k];
    } else {                                     // at an end of the buffer: only what lies inside it is read
#pragma unroll
      for (int k = 0; k < 17; k++) d[k] = sp1_dword_guarded(al + 4 * k, lo, hi);
    }
  }
  uint32_t w[16];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint64_t p = pos + 4 * j;              // message position of the word's first byte
    const uint32_t x = __builtin_bswap32(sha_alignbyte(d[j + 1], d[j], sh));
    const uint32_t kk = (uint32_t)(len - p) & 3; // bytes of the message in this word when p <= len < p + 4
    const uint32_t keep = kk ? 0xFFFFFFFFu << (32 - 8 * kk) : 0u;
    const uint32_t edge = (x & keep) | (0x80000000u >> (8 * kk));
    w[j] = p + 4 <= len ? x : (p <= len ? edge : 0u);
  }
  const uint64_t bits = len * 8;
  const bool last = blk + 1 == nb;
  w[14] = last ? (uint32_t)(bits >> 32) : w[14];
  w[15] = last ? (uint32_t)bits : w[15];
  uint32_t g[8];
#pragma unroll
  for (int k = 0; k < 8; k++) g[k] = h[k];
  sha256_compress(g, w);
  const bool live = blk < nb;
#pragma unroll
  for (int k = 0; k < 8; k++) h[k] = live ? g[k] : h[k];
}

// the digest as the row stores it: eight dwords whose little-endian bytes are the big-endian digest, top three bits of byte 0 cleared
SHA_HD void sp1_digest_words(const uint32_t h[8], uint32_t out[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = __builtin_bswap32(k == 0 ? (h[0] & 0x1FFFFFFFu) : h[k]);
}

// the whole rule for one message, block by block (the host's loop; the kernel runs the same block function under a wavefront-uniform loop)
SHA_HD void sp1_digest(const uint8_t* buf, uint64_t buf_bytes, uint64_t start, uint64_t len, uint32_t out[8]) {
  uint32_t h[8];
  sha256_init(h);
  const uint64_t nb = sha256_blocks(len);
  for (uint64_t b = 0; b < nb; b++) sp1_sha256_block(h, buf, buf_bytes, start, len, b);
  sp1_digest_words(h, out);
}

// the 32-byte vkey hash at p, as eight dwords of its bytes in order (dword loads when p is 4-byte aligned)
SHA_HD void sp1_load_vkey_hash(const uint8_t* p, uint32_t out[8]) {
  if (((uintptr_t)p & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = ((const uint32_t*)p)[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
  }
}

// One whole row, block loop and all (the host's form: bn254_dbg_sp1_public_inputs(device = -1), the host build's launcher): vkey hash at vkh_i, values
// [o0 - base, o1 - base) of pv -> row (16 dwords: vkey hash | digest, as the bytes lie in memory); false if the range is not inside the buffer
SHA_HD bool sp1_row(const uint8_t* vkh_i, const uint8_t* pv, uint64_t pv_bytes, uint64_t base, uint64_t o0, uint64_t o1, uint32_t row[16]) {
  uint64_t start, len;
  const bool ok = sp1_range(o0, o1, base, pv_bytes, &start, &len);
  sp1_load_vkey_hash(vkh_i, row);
  sp1_digest(pv, pv_bytes, start, len, row + 8);
  return ok;
}

}  // namespace bn254
