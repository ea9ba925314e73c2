// The batch-opening entries of the KZG batch (csrc/bn254_capi_kzg.hip: bn254_kzg_verify_folded_batch, _device, bn254_kzg_fold_reserve; the probe
// bn254_dbg_kzg_fold_proof) under the sanitizers, in the pattern of hostsan_kzg.cpp: the host half of the library as ONE translation unit with the stand-in HIP runtime
// of hostsan_main.cpp (whose main is set aside) plus the pairing file and the KZG file.  In the place of the launchers stand: for k_kzg_fold_load the host compile of
// the loader (csrc/bn254_kzg.h::kzg_fold_load_record -- the checks, the transcript, the term records) for the first records of every launch and a marker rule for the
// rest; for k_kzg_ident and the pairing batch a marker rule (bit 0 of a pending status byte: "does not verify") -- on the memory the stand-in runtime hands out, so the
// extents of the staged key and records (record lengths that are no multiple of 4 included), the k + 2 / k + 3 term records, rows, scratch, group buffers, workspace and
// status bytes of every launch are checked by AddressSanitizer against what the host code allocated and copied.
//   BN254_PAIRING_PASS=1000 hostsan_kzg_fold
#include "hip/hip_runtime.h"
#define BN254_HOSTSAN_KZG 1
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_pairing.hip"
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_kzg.hip"
#include <thread>

static std::atomic<size_t> g_load_launches{0}, g_weighted_launches{0}, g_largest_launch{0}, g_pair_launches{0};
#define REAL_ITEMS 3      // records per launch that go through the host compile of the loader; the others: first byte 0xEE = pending and "does not verify", else pending
hipError_t bn254_launch_kzg_load(const bn254::KzgLoadArgs& a, hipStream_t) {
  g_launches++; g_load_launches++;
  if (a.weighted) g_weighted_launches++;
  size_t seen = g_largest_launch.load();
  while (a.n > seen && !g_largest_launch.compare_exchange_weak(seen, a.n)) {}
  const int k = a.n_digests;
  if (k < 1 || k > KZG_FOLD_MAX_DIGESTS || a.data_len < 0 || a.data_len > KZG_FOLD_MAX_DATA) return hipErrorInvalidDevice;      // this harness makes no call on plain openings
  const size_t len = KZG_FOLD_LEN(k, a.data_len);
  if (a.n == 0 || a.n > bn254::kzg_fold_max_launch((size_t)k) || !a.key || ((uintptr_t)a.key & 3) || a.stride < len || ((uintptr_t)a.status & 3)) return hipErrorInvalidDevice;
  const int n_terms = KZG_FOLD_TERMS(k, a.weighted);
  (void)a.key[KZG_KEY_DWORDS - 1];                                          // the last dword a run kernel reads
  memset(a.terms, 0x21, a.n * (size_t)n_terms * MSM_TERM_DWORDS * sizeof(int32_t));
  memset(a.flags, 0x22, a.n * (size_t)n_terms);
  memset(a.status, 0x23, (a.n + 3) & ~(size_t)3);                           // the padded words k_g1_sum_affine ORs into
  if (a.dbg) memset(a.dbg, 0x27, 64 * a.n);
  if (a.weighted && a.weights) (void)a.weights[4 * a.n - 1];
  const bool key_ok = bn254::kzg_key_header_ok(a.key);
  const bool aligned = ((((uintptr_t)a.openings) | a.stride) & 3) == 0;     // the kernel's rule: dword loads of the record then
  for (size_t i = 0; i < a.n; i++) {
    const uint8_t* rec = a.openings + i * a.stride;
    (void)rec[len - 1];                                                     // the last byte the loader reads
    uint8_t st;
    if (!key_ok) st = BN254_ST_MALFORMED;
    else if (i < REAL_ITEMS) {
      bn254::PbHostLane w;
      for (auto& x : w.e) x = bn254::fp_zero();
      uint32_t wgt[4] = {1, 0, 0, 0};
      if (a.weighted) { if (a.weights) { for (int q = 0; q < 4; q++) wgt[q] = a.weights[4 * i + q]; wgt[0] |= 1u; } else bn254::kzg_weight(wgt, a.wkey, (uint32_t)i); }
      st = (uint8_t)bn254::kzg_fold_load_record(w, rec, aligned, k, a.data_len, a.key, a.strict, a.weighted ? wgt : nullptr, a.terms + i * (size_t)n_terms * MSM_TERM_DWORDS,
                                                a.flags + i * (size_t)n_terms, a.dbg ? a.dbg + 64 * i : nullptr);
      if (st & BN254_ST_PENDING) st = BN254_ST_PENDING;
    } else st = rec[0] == 0xEE ? (uint8_t)(BN254_ST_PENDING | 1) : (uint8_t)BN254_ST_PENDING;
    a.status[i] = st;
  }
  return hipSuccess;
}
hipError_t bn254_launch_kzg_ident(const int32_t* key, int32_t* ws, uint8_t* status, size_t n, hipStream_t) {
  g_launches++;
  (void)key[KZG_KEY_DWORDS - 1];
  memset(ws, 0x24, n * (size_t)G16_WS_BYTES_PER_PROOF);
  for (size_t i = 0; i < n; i++) if (status[i] & BN254_ST_PENDING) status[i] = (uint8_t)(BN254_ST_PENDING | (status[i] & 1));      // the marker survives
  return hipSuccess;
}
hipError_t bn254_launch_kzg_fetch(const int32_t* ws, const uint8_t* status, size_t n, uint8_t* out_f, uint8_t* out_h, uint8_t* out_inf, hipStream_t) {
  g_launches++;
  (void)ws[n * (size_t)(G16_WS_BYTES_PER_PROOF / 4) - 1]; (void)status[n - 1];
  memset(out_f, 0x25, 64 * n); memset(out_h, 0x26, 64 * n); memset(out_inf, 0, 2 * n);
  return hipSuccess;
}
hipError_t bn254_launch_pairing_batch(const bn254::PairingLaunchArgs& a, hipStream_t) {
  g_launches++; g_pair_launches++;
  if (a.n == 0 || a.n > (size_t)G16_MAX_LAUNCH || a.n_pairs != 2 || !a.one || a.out_gt || !a.skip_load || a.shared_mask != 3u || !a.prepared || ((uintptr_t)a.prepared & 3)) return hipErrorInvalidDevice;
  (void)a.one[12 * BN_NL - 1]; (void)a.prepared[2 * PB_PREP_DWORDS - 1];
  (void)a.ws[a.n * (size_t)(G16_WS_BYTES_PER_PROOF / 4) - 1];
  for (size_t i = 0; i < a.n; i++) if (a.status[i] & BN254_ST_PENDING) a.status[i] = (a.status[i] & 1) ? BN254_ST_REJECT : BN254_ST_ACCEPT;
  return hipSuccess;
}

static std::vector<uint8_t> g1_bytes() {
  std::vector<uint8_t> b(64);
  bn254::G1Aff g; g.x = bn254::fp_one(); g.y = bn254::fp_add(bn254::fp_one(), bn254::fp_one());
  fp_to_be(b.data(), g.x); fp_to_be(b.data() + 32, g.y);
  return b;
}
static std::vector<uint8_t> g2_bytes() {
  std::vector<uint8_t> b(128);
  bn254::G2Aff g; g.x = bn254::fp2_from_limbs(BN_G2_GEN[0], BN_G2_GEN[1]); g.y = bn254::fp2_from_limbs(BN_G2_GEN[2], BN_G2_GEN[3]);
  fp_to_be(b.data(), g.x.c1); fp_to_be(b.data() + 32, g.x.c0); fp_to_be(b.data() + 64, g.y.c1); fp_to_be(b.data() + 96, g.y.c0);
  return b;
}
static std::vector<uint8_t> make_key() {
  std::vector<uint8_t> key(BN254_KZG_KEY_LEN, 0xEE);
  const std::vector<uint8_t> p = g1_bytes(), q = g2_bytes();
  uint8_t st = 0xEE;
  CHECK(bn254_kzg_key_prepare(p.data(), q.data(), q.data(), key.data(), &st) == BN254_OK && st == BN254_ACCEPT);
  return key;
}
// n records of k digests and dl bytes of data at `stride`, in a heap block that ends with the LAST RECORD (not with its stride): a read past a record's end is seen.
// The first three are real: every digest G1 with H the identity (pending; the marker rule accepts it), the last digest off its curve (NOT_ON_CURVE), z = 2^256 - 1
// (pending; strict: NOT_MEMBER).  The others are markers: `reject(i)` records start with 0xEE.  want: under the exact path, for the records hostsan checks
static std::vector<uint8_t> make_records(size_t n, size_t stride, int k, int dl, const std::function<bool(size_t)>& reject, bool strict, std::vector<uint8_t>& want) {
  const size_t len = KZG_FOLD_LEN(k, dl);
  std::vector<uint8_t> buf((n - 1) * stride + len, 0);
  want.assign(n, BN254_ACCEPT);
  const std::vector<uint8_t> p = g1_bytes();
  for (size_t i = 0; i < n; i++) {
    uint8_t* r = buf.data() + i * stride;
    if (i < REAL_ITEMS) {
      for (int j = 0; j < k; j++) memcpy(r + 64 * j, p.data(), 64);
      for (int j = 0; j < k; j++) r[64 * (k + 1) + 32 + 32 * j + 31] = (uint8_t)(j + 1);      // y_j
      for (int q = 0; q < dl; q++) r[96 + 96 * k + q] = (uint8_t)(q * 7 + i);
      if (i == 1) { r[64 * (k - 1) + 63] ^= 1; want[i] = BN254_ERR_NOT_ON_CURVE; }
      if (i == 2) { memset(r + 64 * (k + 1), 0xff, 32); if (strict) want[i] = BN254_ERR_NOT_MEMBER; }
    } else if (reject(i)) { r[0] = 0xEE; want[i] = BN254_REJECT; }
  }
  return buf;
}

int main() {
  g_fake_device_count = 48;
  const std::vector<uint8_t> key = make_key();
  const auto never = [](size_t) { return false; };
  const int MAXK = BN254_KZG_FOLD_MAX_DIGESTS;
  // ---- the argument checks: BN254_E_BAD_ARG before a device is looked at (ordinal 99 does not exist), nothing written, no launch
  {
    const size_t len = BN254_KZG_FOLD_LEN(3, 5);
    std::vector<uint8_t> item(len * 2), st(2, 0xEE);
    auto clean = [&] { for (auto b : st) if (b != 0xEE) return false; return true; };
    CHECK(bn254_kzg_verify_folded_batch(nullptr, item.data(), len, 1, 3, 5, st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_kzg_verify_folded_batch(key.data(), item.data(), len - 1, 1, 3, 5, st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_kzg_verify_folded_batch(key.data(), item.data(), len, 1, 0, 5, st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_kzg_verify_folded_batch(key.data(), item.data(), 4096, 1, (size_t)MAXK + 1, 0, st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_kzg_verify_folded_batch(key.data(), item.data(), 4096, 1, 3, BN254_KZG_FOLD_MAX_DATA + 1, st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_kzg_verify_folded_batch(key.data(), item.data(), len, 1, 3, 5, st.data(), 99, 4) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_kzg_verify_folded_batch_device(key.data() + 2, item.data(), len, 1, 3, 5, st.data(), 99, nullptr, 0) == BN254_E_BAD_ARG && clean());       // alignment
    CHECK(bn254_kzg_verify_folded_batch_device(key.data(), item.data(), len, 1, 3, 5, nullptr, 99, nullptr, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_kzg_fold_reserve(10, 0, 99) == BN254_E_BAD_ARG && bn254_kzg_fold_reserve(10, (size_t)MAXK + 1, 99) == BN254_E_BAD_ARG);
    CHECK(bn254_kzg_verify_folded_batch(nullptr, nullptr, len, 0, 3, 5, nullptr, 99, BN254_FLAG_RLC) == BN254_OK);
    CHECK(bn254_kzg_verify_folded_batch(key.data(), item.data(), len, 1, 3, 5, st.data(), 99, 0) == BN254_E_BAD_ARG && clean());      // past the argument checks: the device ordinal
    CHECK(g_load_launches.load() == 0);
  }
  // ---- host calls of three passes at k = 1, 3 and the largest k, packed and padded records, data lengths that are and are not multiples of 4, exact and strict: the key
  // staged in front of every pass's records, no launch above the workspace
  for (int k : {1, 3, MAXK})
    for (int dl : {0, 5})
      for (size_t pad : {(size_t)0, (size_t)9})
        for (unsigned flags : {0u, (unsigned)BN254_FLAG_STRICT_SCALARS}) {
          const size_t pass = 1000, n = 2 * pass + 37, stride = BN254_KZG_FOLD_LEN(k, dl) + pad;
          std::vector<uint8_t> want, buf = make_records(n, stride, k, dl, [](size_t i) { return i % 7 == 3; }, flags != 0, want), st(n + 1, 0xEE);
          const size_t before = g_load_launches.load(), pbefore = g_pair_launches.load();
          CHECK(bn254_kzg_verify_folded_batch(key.data(), buf.data(), stride, n, (size_t)k, (size_t)dl, st.data(), 0, flags) == 0 && st[n] == 0xEE);
          CHECK(g_load_launches.load() - before == 3 && g_pair_launches.load() - pbefore == 3 && g_largest_launch.load() <= pass);
          for (size_t i = 0; i < n; i++) if (i < REAL_ITEMS || i % pass >= REAL_ITEMS) CHECK(st[i] == want[i]);
        }
  // the probe's host compile on the real records: the loader's statuses, the digest and y^ only for what reaches the pairing, nothing written past the buffers
  for (int k : {1, MAXK}) {
    const size_t len = BN254_KZG_FOLD_LEN(k, 7);
    std::vector<uint8_t> want, buf = make_records(3, len, k, 7, never, false, want), st(3, 0xEE), fold(64 * 3 + 1, 0xEE), f(64 * 3 + 1, 0xEE), h(64 * 3 + 1, 0xEE), inf(6 + 1, 0xEE), grp(131 + 1, 0xEE);
    CHECK(bn254_dbg_kzg_fold_proof(key.data(), buf.data(), len, 3, (size_t)k, 7, nullptr, 0, fold.data(), f.data(), h.data(), inf.data(), st.data(), nullptr, -1, 0) == 0);
    CHECK(st[1] == BN254_ERR_NOT_ON_CURVE && (st[0] == BN254_ACCEPT || st[0] == BN254_REJECT) && fold[64 * 3] == 0xEE && f[64 * 3] == 0xEE && h[64 * 3] == 0xEE && inf[6] == 0xEE);
    bool any = false, none = true;
    for (int q = 0; q < 32; q++) { any |= fold[q] != 0; none &= fold[64 + q] == 0 && fold[64 + 32 + q] == 0; }
    CHECK(any && none && inf[1] == 1);      // record 0 has a digest and H the identity; record 1 is decided: zero bytes
    CHECK(bn254_dbg_kzg_fold_proof(key.data(), buf.data(), len, 3, (size_t)k, 7, nullptr, BN254_FLAG_RLC, fold.data(), f.data(), h.data(), inf.data(), st.data(), grp.data(), -1, 0) == 0 && grp[131] == 0xEE);
    CHECK(bn254_dbg_kzg_fold_proof(key.data(), buf.data(), len, 3, (size_t)k, 7, nullptr, 0, fold.data(), f.data(), h.data(), inf.data(), st.data(), grp.data(), -1, 0) == BN254_E_BAD_ARG);
  }
  // ---- the device entry: a reservation, then calls at and above it on a stream of the caller's -- at or below the reservation NOTHING is allocated; a corrupted key
  // makes every record MALFORMED
  for (int k : {3, MAXK}) {
    const int dev = k == 3 ? 1 : 2;
    const size_t stride = BN254_KZG_FOLD_LEN(k, 6) + 2;
    CHECK(bn254_kzg_fold_reserve(100, (size_t)k, dev) == 0);
    hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    for (size_t n : {(size_t)1, (size_t)100, (size_t)250}) {
      std::vector<uint8_t> want, buf = make_records(n, stride, k, 6, [](size_t i) { return i % 5 == 4; }, false, want), st(n + 1, 0xEE);
      const size_t live = g_fake_live_allocs.load();
      CHECK(bn254_kzg_verify_folded_batch_device(key.data(), buf.data(), stride, n, (size_t)k, 6, st.data(), dev, s, 0) == 0 && st[n] == 0xEE);
      CHECK(n > 100 || g_fake_live_allocs.load() == live);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    std::vector<uint8_t> bad = key; bad[0] ^= 1;
    std::vector<uint8_t> want, buf = make_records(70, stride, k, 6, never, false, want), st(71, 0xEE);
    CHECK(bn254_kzg_verify_folded_batch_device(bad.data(), buf.data(), stride, 70, (size_t)k, 6, st.data(), dev, s, 0) == 0 && st[70] == 0xEE);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == BN254_ERR_MALFORMED);
    CHECK(bn254_kzg_verify_folded_batch_device(key.data(), buf.data(), stride, 70, (size_t)k, 6, st.data(), dev, s, 0) == 0);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == want[i]);
    hipStreamDestroy(s);
  }
  // ---- BN254_FLAG_RLC with a failing group (the stand-in scatter fails group 3 of every 16): its records go through the per-record check, the others are accepted by
  // their groups; the counters advance as for plain openings
  {
    bn254_set_kzg_params(0);
    const int k = 3;
    const size_t n = 64 * 5 + 10, len = BN254_KZG_FOLD_LEN(k, 5);
    const auto in_group3 = [](size_t i) { return i / 64 == 3 && i % 3 == 1; };
    std::vector<uint8_t> want, buf = make_records(n, len, k, 5, in_group3, false, want), st(n + 1, 0xEE);
    uint64_t s0[4], s1[4];
    CHECK(bn254_kzg_state(s0) == 0);
    const size_t wbefore = g_weighted_launches.load(), pbefore = g_pair_launches.load();
    CHECK(bn254_kzg_verify_folded_batch(key.data(), buf.data(), len, n, (size_t)k, 5, st.data(), 3, BN254_FLAG_RLC) == 0 && st[n] == 0xEE);
    CHECK(bn254_kzg_state(s1) == 0 && s1[0] - s0[0] == 1 && s1[1] - s0[1] == 6 && s1[2] - s0[2] == 1 && s1[3] == s0[3]);
    CHECK(g_weighted_launches.load() - wbefore == 1 && g_pair_launches.load() - pbefore == 2);      // the groups, then the records still pending
    for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    bn254_set_kzg_params((long)n + 1);
    CHECK(bn254_kzg_verify_folded_batch(key.data(), buf.data(), len, n, (size_t)k, 5, st.data(), 3, BN254_FLAG_RLC) == 0);
    uint64_t s2[4];
    CHECK(bn254_kzg_state(s2) == 0 && s2[0] == s1[0] && s2[3] - s1[3] == 1);
    bn254_set_kzg_params(64);
  }
  // ---- an allocation failure at every allocation of a call, each on a device of its own that has passed its self-test: an error code, nothing written, and the same
  // call repeated without the failure answers right (nothing stale, nothing freed twice; leak detection is on)
  for (unsigned flags : {0u, (unsigned)BN254_FLAG_RLC}) {
    const int k = MAXK;
    const size_t n = 70, len = BN254_KZG_FOLD_LEN(k, 5);
    std::vector<uint8_t> want, buf = make_records(n, len, k, 5, [](size_t i) { return i == 9; }, false, want);
    if (flags) want[9] = BN254_ACCEPT;      // group 0 passes in the stand-in: its records are accepted
    bool through = false;
    int dev = flags ? 24 : 4;
    for (size_t fail = 1; fail < 40 && !through; fail++, dev++) {
      unsigned m = 0; float ms = 0;
      CHECK(bn254_device_selftest(dev, &m, &ms) == 0);
      std::vector<uint8_t> st(n + 1, 0xEE);
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      const int rc = bn254_kzg_verify_folded_batch(key.data(), buf.data(), len, n, (size_t)k, 5, st.data(), dev, flags);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) through = true;
      else { CHECK(rc == BN254_E_NOMEM); for (auto b : st) CHECK(b == 0xEE); }
      CHECK(bn254_kzg_verify_folded_batch(key.data(), buf.data(), len, n, (size_t)k, 5, st.data(), dev, flags) == 0 && st[n] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    CHECK(through && dev > (flags ? 24 : 4) + 8);
  }
  // ---- two host threads on one device, one through the host entry and one through the device entry, with different k: the device's lock serialises them and the
  // staging and the term records belong to one call at a time
  {
    const int dev = 46;
    std::atomic<int> bad{0};
    auto worker = [&](int which) {
      const int k = which ? MAXK : 2;
      const size_t stride = BN254_KZG_FOLD_LEN(k, 3) + (which ? 0 : 4);
      for (int it = 0; it < 12; it++) {
        const size_t n = 30 + 17 * (size_t)it + (size_t)which;
        std::vector<uint8_t> want, buf = make_records(n, stride, k, 3, [&](size_t i) { return (i + (size_t)which) % 4 == 0; }, false, want), st(n, 0xEE);
        const int rc = which ? bn254_kzg_verify_folded_batch_device(key.data(), buf.data(), stride, n, (size_t)k, 3, st.data(), dev, nullptr, 0)
                             : bn254_kzg_verify_folded_batch(key.data(), buf.data(), stride, n, (size_t)k, 3, st.data(), dev, 0);
        if (rc != 0 || st != want) bad++;
      }
    };
    std::thread t0(worker, 0), t1(worker, 1);
    t0.join(); t1.join();
    CHECK(bad.load() == 0);
  }
  printf("hostsan_kzg_fold: %zu stand-in launches of the fold loader (%zu weighted), the largest of %zu records, %zu pairing launches, %zu allocations still live (the per-device buffers)\nhostsan_kzg_fold ok\n",
         g_load_launches.load(), g_weighted_launches.load(), g_largest_launch.load(), g_pair_launches.load(), g_fake_live_allocs.load());
  return 0;
}
