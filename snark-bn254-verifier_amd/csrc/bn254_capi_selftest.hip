// bn254_capi_selftest.hip -- the host half of the device self-test (include/bn254_verify.h: bn254_device_selftest, bn254_device_selftest_state,
// bn254_selftest_check_name; BN254_SELFTEST): the built-in vectors and their expected values, the comparison and its text, the per-device state, the gate every
// path that makes a device ready passes (selftest_gate, bn254_capi_internal.h), the entries and the probes of the tests.  The device half is
// bn254_selftest_dev.hip (bn254_selftest.h has the layouts).
//
// Where the expected values come from.  Statuses of the Groth16 and two-pair checks: tables of gen_constants.py (csrc/bn254_constants.h, BN_ST_*), made from the
// key's trapdoors in Python integers, so no pairing is computed for them anywhere; tests/test_selftest_cpu.py holds them against the oracle.  Everything else: the host's
// compile of the arithmetic the kernels run (bn254_pairing.h, bn254_codec.h, bn254_sha256.h), computed once per process WHILE the device runs the first self-test.
#if !defined(BN254_SELFTEST_TABLES)
#define BN254_SELFTEST_TABLES 1
#endif
#include "bn254_selftest.h"
#include "bn254_sha256.h"

using namespace bn254st;

static_assert(sizeof(BN_ST_VK) == VK_LEN && sizeof(BN_ST_PROOFS) == G16_N * 256 && sizeof(BN_ST_INPUTS) == G16_N * 64 && sizeof(BN_ST_STATUS) == G16_N &&
              sizeof(BN_ST_PAIR2) == P2_N * 128 && sizeof(BN_ST_PAIR2_FLAGS) == P2_N && sizeof(BN_ST_PAIR2_STATUS) == P2_N && BN_ST_N == 64,
              "self-test tables out of sync with bn254_selftest.h");

namespace {
const char* const CHECK_NAME[CK_COUNT] = {"fp", "fp12_lane", "fp12_coop", "pairing_lane", "g16_lane", "g16_coop", "pair2_lane", "pair2_coop", "codec", "sha256"};
// BN254_SELFTEST=0 skips the automatic run (read once, when the library is loaded)
const bool g_auto = [] { const char* e = getenv("BN254_SELFTEST"); return !e || atoi(e) != 0; }();

// ---------------------------------------------------------------- Fp12 values as the probes carry them: 12 x 32 bytes, tower order
Fp12 f12_from_bytes(const uint8_t* b) {
  Fp12 f;
  Fp2* t[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int i = 0; i < 6; i++) { t[i]->c0 = fp_from_be(b + 64 * i); t[i]->c1 = fp_from_be(b + 64 * i + 32); }
  return f;
}
void f12_to_bytes(uint8_t* b, const Fp12& f) {
  const Fp2* t[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int i = 0; i < 6; i++) { fp_to_be(b + 64 * i, t[i]->c0); fp_to_be(b + 64 * i + 32, t[i]->c1); }
}
void rand_fp(SplitMix64& g, uint8_t* out32) {      // a canonical value below p
  uint8_t b[32];
  for (int i = 0; i < 4; i++) { const uint64_t v = g.next(); for (int j = 0; j < 8; j++) b[8 * i + j] = (uint8_t)(v >> (8 * j)); }
  fp_to_be(out32, fp_from_be(b));
}
void rand_f12(SplitMix64& g, uint8_t* out384) { for (int i = 0; i < 12; i++) rand_fp(g, out384 + 32 * i); }
G1Aff g1_from_bytes(const uint8_t* b) { G1Aff p; p.x = fp_from_be(b); p.y = fp_from_be(b + 32); return p; }
G2Aff g2_from_bytes(const uint8_t* b) { G2Aff q; q.x.c1 = fp_from_be(b); q.x.c0 = fp_from_be(b + 32); q.y.c1 = fp_from_be(b + 64); q.y.c0 = fp_from_be(b + 96); return q; }

// ---------------------------------------------------------------- the vectors: inputs at the first use, the key and the expected values when they are first needed
struct Vectors {
  std::vector<uint8_t> in[CK_COUNT], expect[CK_COUNT];
  G16Key vk; Key key;
  std::once_flag key_once, expect_once;
  bool vk_ok = false, key_ok = false;
};
void build_inputs(Vectors& v) {
  SplitMix64 g{0x5e1f7e57b254a001ull};
  for (int k = 0; k < CK_COUNT; k++) v.in[k].assign(in_bytes(k), 0);
  // fp: 0, 1, p - 1, p - 2, all-ones and alternating digits against each other, then pseudo-random pairs
  {
    uint8_t sp[7][32];
    memset(sp, 0, sizeof sp);
    sp[1][31] = 1;
    uint32_t w[8];
    memcpy(w, BN_P_WORDS, sizeof w); w[0] -= 1; words_to_be(sp[2], w);      // p is odd: no borrow
    w[0] -= 1; words_to_be(sp[3], w);
    memset(sp[4], 0xff, 32); sp[4][0] = 0x0f;
    memset(sp[5], 0xaa, 32); sp[5][0] = 0x2a;
    memset(sp[6], 0x55, 32); sp[6][0] = 0x15;
    uint8_t* a = v.in[CK_FP].data(); uint8_t* b = a + FP_N * 32;
    for (int i = 0; i < FP_N; i++) {
      if (i < 14) { memcpy(a + 32 * i, sp[i % 7], 32); memcpy(b + 32 * i, sp[(i % 7 + 2 + i / 7) % 7], 32); }
      else { rand_fp(g, a + 32 * i); rand_fp(g, b + 32 * i); }
    }
  }
  // Fp12: random values, and cyclotomic ones (the easy part of the final exponentiation of a random value)
  for (int k : {(int)CK_FP12_LANE, (int)CK_FP12_COOP}) {
    const int n = k == CK_FP12_LANE ? F12L_N : F12C_N;
    uint8_t* a = v.in[k].data();
    for (int i = 0; i < 2 * n; i++) rand_f12(g, a + 384 * i);
    for (int i = 0; i < n; i++) { uint8_t t[384]; rand_f12(g, t); f12_to_bytes(a + 384 * (2 * n + i), final_exp_easy(f12_from_bytes(t))); }
  }
  // pairings: e(G1, G2), e(a G1, b G2) and e(-a G1, b G2) from the first built-in proof, A and B of the second
  {
    uint8_t* g1 = v.in[CK_PAIRING_LANE].data(); uint8_t* g2 = g1 + PAIR_N * 64;
    G1Aff gen; gen.x = fp_one(); gen.y = fp_add(fp_one(), fp_one());
    G2Aff gen2; gen2.x = fp2_from_limbs(BN_G2_GEN[0], BN_G2_GEN[1]); gen2.y = fp2_from_limbs(BN_G2_GEN[2], BN_G2_GEN[3]);
    enc_g1_uncompressed(g1, gen); enc_g2_uncompressed(g2, gen2);
    memcpy(g1 + 64, BN_ST_PROOFS, 64); memcpy(g2 + 128, BN_ST_PROOFS + 64, 128);
    enc_g1_uncompressed(g1 + 128, g1_neg(g1_from_bytes(BN_ST_PROOFS))); memcpy(g2 + 256, BN_ST_PROOFS + 64, 128);
    memcpy(g1 + 192, BN_ST_PROOFS + 256, 64); memcpy(g2 + 384, BN_ST_PROOFS + 256 + 64, 128);
  }
  // Groth16: the tables
  for (int k : {(int)CK_G16_LANE, (int)CK_G16_COOP}) {
    uint8_t* p = v.in[k].data();
    memcpy(p, BN_ST_VK, VK_LEN); memcpy(p + VK_LEN, BN_ST_PROOFS, sizeof BN_ST_PROOFS); memcpy(p + VK_LEN + sizeof BN_ST_PROOFS, BN_ST_INPUTS, sizeof BN_ST_INPUTS);
  }
  // the two-pair check: the G2 points the key's line tables are made of (prepare_g16, reference mode: gamma as decoded, delta negated), 1 in GT, the items
  v.vk_ok = parse_g16_vk(v.vk, BN_ST_VK, VK_LEN, BN254_VK_REFERENCE) == DEC_OK;
  for (int k : {(int)CK_PAIR2_LANE, (int)CK_PAIR2_COOP}) {
    uint8_t* p = v.in[k].data();
    if (v.vk_ok) { enc_g2_uncompressed(p, v.vk.gamma); enc_g2_uncompressed(p + 128, g2_neg(v.vk.delta)); }
    p[256 + 31] = 1;
    for (int i = 0; i < P2_N; i++) { memcpy(p + 640 + 64 * i, BN_ST_PAIR2 + 128 * i, 64); memcpy(p + 640 + P2_N * 64 + 64 * i, BN_ST_PAIR2 + 128 * i + 64, 64); }
    memcpy(p + 640 + P2_N * 128, BN_ST_PAIR2_FLAGS, P2_N);
  }
  // codec: the first eight proofs compressed; then flag 0b00 on A, an x without a square root (0: 3 is a non-residue), the G2 infinity flag (the generator)
  {
    uint8_t* r = v.in[CK_CODEC].data();
    for (int i = 0; i < 8; i++) {
      const uint8_t* p = BN_ST_PROOFS + 256 * i;
      enc_g1_compressed(r + 128 * i, g1_from_bytes(p)); enc_g2_compressed(r + 128 * i + 32, g2_from_bytes(p + 64)); enc_g1_compressed(r + 128 * i + 96, g1_from_bytes(p + 192));
    }
    memcpy(r + 128 * 8, r, 128); r[128 * 8] &= 0x3f;
    memcpy(r + 128 * 9, r + 128, 128); memset(r + 128 * 9, 0, 32); r[128 * 9] = 0x80;
    memcpy(r + 128 * 10, r + 256, 128); memset(r + 128 * 10 + 32, 0, 64); r[128 * 10 + 32] = 0x40;
  }
  // SHA-256: values of 0, 55, 56, 64, 119, 120 and 1000 bytes one after the other from byte 3 on (every padding case, no value aligned), and a last range that
  // ends outside the buffer
  {
    uint8_t* p = v.in[CK_SHA256].data();
    for (int i = 0; i < SHA_N * 32; i++) p[i] = (uint8_t)g.next();
    static const uint64_t len[SHA_N - 1] = {0, 55, 56, 64, 119, 120, 1000};
    uint64_t off[SHA_N + 1], pv_bytes = SHA_PV_BYTES;
    off[0] = 3;
    for (int i = 0; i < SHA_N - 1; i++) off[i + 1] = off[i] + len[i];
    off[SHA_N] = 5000;
    memcpy(p + SHA_N * 32, off, sizeof off); memcpy(p + SHA_N * 32 + sizeof off, &pv_bytes, 8);
    uint8_t* pv = p + SHA_N * 32 + sizeof off + 8;
    for (int i = 0; i < SHA_PV_BYTES; i++) pv[i] = (uint8_t)g.next();
  }
}
Vectors& vectors() {
  static Vectors* v = [] { Vectors* x = new Vectors(); build_inputs(*x); return x; }();      // never destroyed: a self-test may run while the process exits
  return *v;
}
const Key* vectors_key() {
  Vectors& v = vectors();
  std::call_once(v.key_once, [&v] {
    G16Prepared h;
    if (!v.vk_ok || !prepare_g16(h, v.vk, BN254_VK_REFERENCE) || h.kpts.size() != 2 * 2 * BN_NL) return;
    v.key.k0 = h.k0; v.key.gtab = h.gtab; v.key.dtab = h.dtab; v.key.target = h.target; v.key.kpts = h.kpts;
    v.key.one.resize(12 * BN_NL);
    put_fp12(v.key.one.data(), fp12_one());
    v.key_ok = true;
  });
  if (!v.key_ok) { set_err(BN254_E_VK, "the built-in key of the self-test does not load"); return nullptr; }
  return &v.key;
}
void build_expected(Vectors& v) {
  for (int k = 0; k < CK_COUNT; k++) v.expect[k].assign(out_bytes(k), 0);
  {
    const uint8_t* a = v.in[CK_FP].data(); const uint8_t* b = a + FP_N * 32;
    for (int i = 0; i < FP_N; i++) fp_to_be(v.expect[CK_FP].data() + 32 * i, fp_mul(fp_from_be(a + 32 * i), fp_from_be(b + 32 * i)));
  }
  {
    const uint8_t* a = v.in[CK_FP12_LANE].data();
    uint8_t* o = v.expect[CK_FP12_LANE].data();
    for (int i = 0; i < F12L_N; i++) {
      const Fp12 x = f12_from_bytes(a + 384 * i), y = f12_from_bytes(a + 384 * (F12L_N + i)), c = f12_from_bytes(a + 384 * (2 * F12L_N + i));
      const Fp12 r[F12L_OPS] = {fp12_mul(x, y), fp12_sqr(x), fp12_inv(x), fp12_cyclo_sqr(final_exp_easy(x)), fp12_frob(x, 1), fp12_cyclo_sqr(c), fp12_frob(x, 2), fp12_frob(x, 3)};
      for (int op = 0; op < F12L_OPS; op++) f12_to_bytes(o + 384 * ((size_t)op * F12L_N + i), r[op]);
    }
  }
  {
    const uint8_t* a = v.in[CK_FP12_COOP].data();
    uint8_t* o = v.expect[CK_FP12_COOP].data();
    for (int i = 0; i < F12C_N; i++) {
      const Fp12 x = f12_from_bytes(a + 384 * i), y = f12_from_bytes(a + 384 * (F12C_N + i)), c = f12_from_bytes(a + 384 * (2 * F12C_N + i));
      const Fp12 r[F12C_OPS] = {fp12_mul(x, y), fp12_sqr(x), fp12_cyclo_sqr(fp12_cyclo_sqr(fp12_cyclo_sqr(c))), fp12_frob(x, 1), fp12_frob(x, 2), fp12_frob(x, 3), fp12_inv(x),
                                final_exponentiation(x)};
      for (int op = 0; op < F12C_OPS; op++) f12_to_bytes(o + 384 * ((size_t)op * F12C_N + i), r[op]);
    }
  }
  {
    const uint8_t* g1 = v.in[CK_PAIRING_LANE].data(); const uint8_t* g2 = g1 + PAIR_N * 64;
    for (int i = 0; i < PAIR_N; i++)
      f12_to_bytes(v.expect[CK_PAIRING_LANE].data() + 384 * i, final_exponentiation(miller_loop<0>(g1_from_bytes(g1 + 64 * i), g2_from_bytes(g2 + 128 * i), nullptr, nullptr)));
  }
  for (int k : {(int)CK_G16_LANE, (int)CK_G16_COOP}) memcpy(v.expect[k].data(), BN_ST_STATUS, G16_N);
  for (int k : {(int)CK_PAIR2_LANE, (int)CK_PAIR2_COOP}) memcpy(v.expect[k].data(), BN_ST_PAIR2_STATUS, P2_N);
  {
    uint8_t* o = v.expect[CK_CODEC].data();
    for (int i = 0; i < CODEC_N; i++) {
      uint32_t rec[32], raw[64];
      memcpy(rec, v.in[CK_CODEC].data() + 128 * i, 128);
      o[CODEC_N * 256 + i] = g16_decompress_record(rec, raw) ? 0 : 1;
      memcpy(o + 256 * i, raw, 256);
    }
  }
  {
    const uint8_t* p = v.in[CK_SHA256].data();
    uint64_t off[SHA_N + 1], pv_bytes;
    memcpy(off, p + SHA_N * 32, sizeof off); memcpy(&pv_bytes, p + SHA_N * 32 + sizeof off, 8);
    // the values in a buffer of their own, dword-aligned as the device copy is
    std::vector<uint32_t> pv((SHA_PV_BYTES + 3) / 4 + 1);
    memcpy(pv.data(), p + SHA_N * 32 + sizeof off + 8, SHA_PV_BYTES);
    uint8_t* o = v.expect[CK_SHA256].data();
    for (int i = 0; i < SHA_N; i++) {
      uint32_t row[16];
      o[SHA_N * 64 + i] = bn254::sp1_row(p + 32 * i, (const uint8_t*)pv.data(), pv_bytes, 0, off[i], off[i + 1], row) ? 0 : 1;
      memcpy(o + 64 * i, row, 64);
    }
  }
}
const Vectors& vectors_expected() {
  Vectors& v = vectors();
  std::call_once(v.expect_once, [&v] { build_expected(v); });
  return v;
}

// the byte of check k's input whose low bit a fault injection flips (bn254_dbg_selftest): one that changes what the kernels compute -- for the status checks, a
// proof's status
size_t corrupt_byte(int k) {
  switch (k) {
    case CK_FP: return 32 * 20 + 31;                                   // a pseudo-random operand
    case CK_FP12_LANE: case CK_FP12_COOP: return 31;                   // the first number of the first value a
    case CK_PAIRING_LANE: return 64 + 31;                              // x of the second pair's G1 point
    case CK_G16_LANE: case CK_G16_COOP: return VK_LEN + G16_N * 256 + 31;      // the first input of proof 0 (valid): REJECT
    case CK_PAIR2_LANE: case CK_PAIR2_COOP: return 640 + 31;           // x of P_0 of item 0 (accepted): the product is no longer 1
    case CK_CODEC: return 31;                                          // x of A of the first record
    case CK_SHA256: return SHA_N * 32 + (SHA_N + 1) * 8 + 8 + 3 + 10;  // a byte of the second value
  }
  return 0;
}

// ---------------------------------------------------------------- one run
struct Report { unsigned mask = 0; std::string text; float ms = 0.f; float gpu_ms[MS_COUNT] = {0}; float host_ms = 0.f; };
std::mutex g_last_mu;
Report g_last;      // the last run of the process, for bn254_dbg_selftest_ms

std::string hex8(const uint8_t* p, size_t n) {
  char t[3]; std::string s;
  for (size_t i = 0; i < n && i < 8; i++) { snprintf(t, sizeof t, "%02x", p[i]); s += t; }
  return s + "..";
}
// caller made `device` current (check_device).  BN254_OK: the run was made, rep says what it found
int run_checks(int device, int corrupt_check, Report& rep) {
  const auto t0 = std::chrono::steady_clock::now();
  const Vectors& v = vectors();
  std::vector<uint8_t> in[CK_COUNT], got[CK_COUNT];
  for (int k = 0; k < CK_COUNT; k++) in[k] = v.in[k];
  if (corrupt_check >= 0 && corrupt_check < CK_COUNT) in[corrupt_check][corrupt_byte(corrupt_check)] ^= 1;
  double host_ms = 0;
  auto timed = [&host_ms](const std::function<void()>& f) {
    const auto a = std::chrono::steady_clock::now();
    f();
    host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
  };
  HostSide hs;
  hs.key = [&]() { const Key* k = nullptr; timed([&k] { k = vectors_key(); }); return k; };
  hs.overlap = [&]() { timed([] { (void)vectors_expected(); }); };
  const int rc = bn254_selftest_device(device, in, hs, got, rep.gpu_ms);
  if (rc) return rc;
  const Vectors& x = vectors_expected();
  rep.mask = 0; rep.text.clear();
  for (int k = 0; k < CK_COUNT; k++) {
    const std::vector<uint8_t>& e = x.expect[k];
    if (got[k].size() == e.size() && memcmp(got[k].data(), e.data(), e.size()) == 0) continue;
    rep.mask |= 1u << k;
    if (!rep.text.empty()) continue;
    size_t at = 0;
    while (at < e.size() && at < got[k].size() && got[k][at] == e[at]) at++;
    const size_t unit = (k == CK_G16_LANE || k == CK_G16_COOP || k == CK_PAIR2_LANE || k == CK_PAIR2_COOP) ? 1 : 32, lo = at / unit * unit;
    rep.text = "device self-test failed on device " + std::to_string(device) + " (a shipped kernel on this GPU disagrees with its known answer) -- check " + std::to_string(k) +
               " (" + CHECK_NAME[k] + "), output byte " + std::to_string(at) + ": device " + (lo < got[k].size() ? hex8(got[k].data() + lo, got[k].size() - lo) : std::string("nothing")) +
               " expected " + (lo < e.size() ? hex8(e.data() + lo, e.size() - lo) : std::string("nothing"));
  }
  rep.host_ms = (float)host_ms;
  rep.ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  { std::lock_guard<std::mutex> lk(g_last_mu); g_last = rep; }
  return BN254_OK;
}

// ---------------------------------------------------------------- per-device state and the gate
#define SELFTEST_MAX_DEVICES 64     // as bn254_shard_plan
struct Slot {
  std::mutex mu;                    // held for a run: concurrent first calls wait for the one run
  std::atomic<int> state{-1};       // -1 not run, 0 failed, 1 passed, 2 skipped (BN254_SELFTEST=0)
  unsigned mask = 0; std::string text;      // of the recorded run (under mu)
};
Slot g_slot[SELFTEST_MAX_DEVICES];

// One run on `device` (current), the caller holding s.mu.  BN254_OK: every check agrees; BN254_E_SELFTEST: one does not (*failed_mask says which, bn254_last_error()
// names the first); any other code: the run could not be made, and nothing is recorded -- the next call tries again
int run_and_record(Slot& s, int device, int corrupt_check, bool record, unsigned* failed_mask, float* ms) {
  Report rep;
  const int rc = run_checks(device, corrupt_check, rep);
  if (rc) return rc;
  if (failed_mask) *failed_mask = rep.mask;
  if (ms) *ms = rep.ms;
  if (record) { s.mask = rep.mask; s.text = rep.text; s.state.store(rep.mask ? 0 : 1, std::memory_order_release); }
  return rep.mask ? set_err(BN254_E_SELFTEST, rep.text) : BN254_OK;
}
int explicit_run(int device, int corrupt_check, bool record, unsigned* failed_mask, float* ms) {
  if (failed_mask) *failed_mask = 0;
  if (ms) *ms = 0.f;
  int rc = check_device(device);
  if (rc) return rc;
  if (device >= SELFTEST_MAX_DEVICES) return set_err(BN254_E_BAD_ARG, "device ordinal out of range");
  Slot& s = g_slot[device];
  std::lock_guard<std::mutex> lk(s.mu);
  return run_and_record(s, device, corrupt_check, record, failed_mask, ms);
}
}  // namespace

// Every path that makes a device ready calls this after check_device (ensure_dev, plonk_ensure_dev, the first use of a key list, the device passes of
// bn254_groth16_vk_prepare_batch): the first call per process and device runs the self-test, every later one is one atomic load -- or, on a device that failed,
// BN254_E_SELFTEST with the recorded text.
int selftest_gate(int device) {
  if (device < 0 || device >= SELFTEST_MAX_DEVICES) return set_err(BN254_E_BAD_ARG, "device ordinal out of range");
  Slot& s = g_slot[device];
  int st = s.state.load(std::memory_order_acquire);
  if (st == 1 || st == 2) return BN254_OK;
  std::lock_guard<std::mutex> lk(s.mu);
  st = s.state.load(std::memory_order_acquire);
  if (st == 1 || st == 2) return BN254_OK;
  if (st == 0) return set_err(BN254_E_SELFTEST, s.text);
  if (!g_auto) { s.state.store(2, std::memory_order_release); return BN254_OK; }
  return run_and_record(s, device, -1, true, nullptr, nullptr);
}
// the expected bytes of check k (the stand-in of a host build hands them back as "what the device computed")
const std::vector<uint8_t>& bn254_selftest_expected(int k) { return vectors_expected().expect[k]; }

extern "C" {

const char* bn254_selftest_check_name(int check) { return check >= 0 && check < CK_COUNT ? CHECK_NAME[check] : ""; }

int bn254_device_selftest(int device, unsigned* failed_mask, float* ms) { return explicit_run(device, -1, true, failed_mask, ms); }

int bn254_device_selftest_state(int device, int* state, unsigned* failed_mask) {
  if (device < 0 || device >= SELFTEST_MAX_DEVICES || !state) return set_err(BN254_E_BAD_ARG, "bad argument");
  Slot& s = g_slot[device];
  std::lock_guard<std::mutex> lk(s.mu);
  *state = s.state.load(std::memory_order_acquire);
  if (failed_mask) *failed_mask = *state == 0 ? s.mask : 0;
  return BN254_OK;
}

// ---- probes (tests)
int bn254_dbg_selftest_vectors(int check, uint8_t* in, size_t in_cap, size_t* in_len, uint8_t* expect, size_t exp_cap, size_t* exp_len) {
  if (check < 0 || check >= CK_COUNT || !in_len || !exp_len) return set_err(BN254_E_BAD_ARG, "bad argument");
  *in_len = in_bytes(check); *exp_len = out_bytes(check);
  if (!in || !expect || in_cap < *in_len || exp_cap < *exp_len) return set_err(BN254_E_BAD_ARG, "vector buffer too small");
  const Vectors& v = vectors_expected();
  memcpy(in, v.in[check].data(), *in_len); memcpy(expect, v.expect[check].data(), *exp_len);
  return BN254_OK;
}
int bn254_dbg_selftest(int device, int corrupt_check, int record, unsigned* failed_mask) {
  if (corrupt_check < -1 || corrupt_check >= CK_COUNT || (record & ~1)) return set_err(BN254_E_BAD_ARG, "bad argument");
  return explicit_run(device, corrupt_check, record != 0, failed_mask, nullptr);
}
int bn254_dbg_selftest_ms(float gpu_ms[BN254_SELFTEST_NUM_CHECKS + 1], float* host_ms, float* wall_ms) {
  if (!gpu_ms) return set_err(BN254_E_BAD_ARG, "bad argument");
  std::lock_guard<std::mutex> lk(g_last_mu);
  for (int k = 0; k < MS_COUNT; k++) gpu_ms[k] = g_last.gpu_ms[k];
  if (host_ms) *host_ms = g_last.host_ms;
  if (wall_ms) *wall_ms = g_last.ms;
  return BN254_OK;
}

}  // extern "C"
