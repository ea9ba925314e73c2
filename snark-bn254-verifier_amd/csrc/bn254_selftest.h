// bn254_selftest.h -- what the two halves of the device self-test share (include/bn254_verify.h, bn254_device_selftest): the sizes and the byte layouts of the
// ten checks' inputs and outputs, and the one function of the device half.  Private: nothing outside csrc/ and the harnesses of tests/hostsan includes it.
//
// The host half (bn254_capi_selftest.hip) owns the vectors, the expected values, the comparison, the texts, the gate and the entries.  The device half
// (bn254_selftest_dev.hip) uploads the inputs it is handed, calls the product's launchers, downloads what they wrote -- no arithmetic of its own and no kernel.
// A host build has no device half: bn254_capi.hip's bottom block holds a stand-in that hands the expected bytes back (BN254_HOSTSAN_SELFTEST: the harness brings its own).
#pragma once
#include <functional>
#include <vector>
#include "bn254_capi_internal.h"

namespace bn254st {
enum { CK_FP = 0, CK_FP12_LANE, CK_FP12_COOP, CK_PAIRING_LANE, CK_G16_LANE, CK_G16_COOP, CK_PAIR2_LANE, CK_PAIR2_COOP, CK_CODEC, CK_SHA256, CK_COUNT };
static_assert(CK_COUNT == BN254_SELFTEST_NUM_CHECKS, "check count out of sync with the header");

// Layouts (every Fp12 value: 384 bytes, every G1 point 64, every G2 point 128, as the probes of include/bn254_verify.h take them):
//   fp            in  a[64] | b[64] (32 bytes each)                                           out 64 products
//   fp12_lane     in  a[2] | b[2] | c[2] (c: cyclotomic)                                      out 8 ops x 2: a b, a^2, 1/a, cyclo_sqr(easy(a)), frob1 a, cyclo_sqr(c), frob2 a, frob3 a
//   fp12_coop     in  a[6] | b[6] | c[6]                                                      out 8 ops x 6: a b, a^2, c^(2^3), frob1 a, frob2 a, frob3 a, 1/a, final_exp(a)
//   pairing_lane  in  g1[4] | g2[4]                                                           out 4 GT values
//   g16_lane/coop in  vk (520 bytes, gnark) | 64 raw proofs (256) | 64 input rows (2 x 32)    out 64 status bytes
//   pair2_lane/coop in Q_0 | Q_1 (the G2 points of the key's two line tables) | target | P_0[64] | P_1[64] | 64 flag bytes (bit t: P_t is the identity)
//                                                                                             out 64 status bytes (ACCEPT or BN254_ERR_PAIRING_FAILED)
//   codec         in  11 compressed records (128)                                             out 11 raw records (256) | 11 pre bytes
//   sha256        in  8 vkey hashes (32) | 9 offsets (u64, little-endian) | pv_bytes (u64) | the values' buffer     out 8 rows (64) | 8 pre bytes
enum { FP_N = 64, F12L_N = 2, F12L_OPS = 8, F12C_N = 6, F12C_OPS = 8, PAIR_N = 4, G16_N = 64, VK_LEN = 520, P2_N = 64, CODEC_N = 11, SHA_N = 8, SHA_PV_BYTES = 1424 };
enum { P2_REJECT = BN254_ERR_PAIRING_FAILED };
// the operations of fp12_coop: {op of bn254_coop12_dbg_op, arg, operand: 0 a, 2 c, second operand b?}
struct CoopOp { int op, arg, src, two; };
static const CoopOp F12C_OP[F12C_OPS] = {{0, 0, 0, 1}, {3, 0, 0, 0}, {4, 3, 2, 0}, {5, 1, 0, 0}, {5, 2, 0, 0}, {5, 3, 0, 0}, {6, 0, 0, 0}, {11, 0, 0, 0}};

static inline size_t in_bytes(int k) {
  switch (k) {
    case CK_FP: return 2 * FP_N * 32;
    case CK_FP12_LANE: return 3 * F12L_N * 384;
    case CK_FP12_COOP: return 3 * F12C_N * 384;
    case CK_PAIRING_LANE: return PAIR_N * (64 + 128);
    case CK_G16_LANE: case CK_G16_COOP: return VK_LEN + G16_N * (256 + 64);
    case CK_PAIR2_LANE: case CK_PAIR2_COOP: return 128 + 128 + 384 + P2_N * (64 + 64 + 1);
    case CK_CODEC: return CODEC_N * 128;
    case CK_SHA256: return SHA_N * 32 + (SHA_N + 1) * 8 + 8 + SHA_PV_BYTES;
  }
  return 0;
}
static inline size_t out_bytes(int k) {
  switch (k) {
    case CK_FP: return FP_N * 32;
    case CK_FP12_LANE: return F12L_OPS * F12L_N * 384;
    case CK_FP12_COOP: return F12C_OPS * F12C_N * 384;
    case CK_PAIRING_LANE: return PAIR_N * 384;
    case CK_G16_LANE: case CK_G16_COOP: return G16_N;
    case CK_PAIR2_LANE: case CK_PAIR2_COOP: return P2_N;
    case CK_CODEC: return CODEC_N * 257;
    case CK_SHA256: return SHA_N * 65;
  }
  return 0;
}

// the built-in key as the kernels read it (bn254_host.hpp::G16Prepared of the vk bytes in the g16 checks' input, reference mode) and 1 in GT
struct Key { std::vector<int32_t> k0, gtab, dtab, target, kpts, one; };
// What the host does while the device works: key() after the checks that need no key are enqueued -- the key is prepared on the host meanwhile (null: it failed,
// set_err has the text) -- and overlap() when everything is enqueued: the host computes the expected values it does not have yet
struct HostSide { std::function<const Key*()> key; std::function<void()> overlap; };
enum { MS_KEY = CK_COUNT, MS_COUNT };    // gpu_ms[MS_KEY]: the key's upload and the construction of its window tables
}  // namespace bn254st

// bn254_capi_selftest.hip: the expected output bytes of check k (computed at the first use)
const std::vector<uint8_t>& bn254_selftest_expected(int k);
// Runs the ten checks on `device` (made current by the caller) on a stream of its own: in[k] (in_bytes(k) bytes each) -> got[k] (out_bytes(k) bytes), gpu_ms[k] the time
// between the events around check k.  Synchronises with that stream only and frees everything it allocated.  BN254_OK, or the code of what failed (set_err).
int bn254_selftest_device(int device, const std::vector<uint8_t> in[bn254st::CK_COUNT], const bn254st::HostSide& host, std::vector<uint8_t> got[bn254st::CK_COUNT],
                          float gpu_ms[bn254st::MS_COUNT]);
