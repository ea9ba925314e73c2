// Pairing batches with shared, prepared G2 points (csrc/bn254_capi_pairing.hip: bn254_g2_prepare, bn254_pairing_check_batch_shared, _device,
// bn254_pairing_batch_shared) under the sanitizers, in the pattern of hostsan_pairing.cpp: the host half of the library as ONE translation unit with the stand-in HIP
// runtime of hostsan_main.cpp (whose main is set aside) plus the pairing file.  In the place of bn254_launch_pairing_batch stands the host compile of the kernels'
// bodies (csrc/bn254_pairing_batch.h::pb_item_shared_on_host / pb_item_on_host) for the first items of every launch and a marker rule for the rest, on the memory
// the stand-in runtime hands out -- so the extents of the packed items, of the STAGED prepared records, of the workspace, the status bytes and the GT values of every
// launch are checked by AddressSanitizer against what the host code allocated and copied.
//   BN254_PAIRING_PASS=1000 hostsan_pairing_shared
#include "hip/hip_runtime.h"
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_pairing.hip"
#include <thread>

static std::atomic<size_t> g_pair_launches{0}, g_shared_launches{0}, g_largest_launch{0};
#define REAL_ITEMS 3      // items per launch that go through the host compile of the kernels; the others: first byte 0xEE = REJECT, else ACCEPT
hipError_t bn254_launch_pairing_batch(const bn254::PairingLaunchArgs& a, hipStream_t) {
  g_launches++; g_pair_launches++;
  if (a.shared_mask) g_shared_launches++;
  size_t seen = g_largest_launch.load();
  while (a.n > seen && !g_largest_launch.compare_exchange_weak(seen, a.n)) {}
  if (a.n == 0 || a.n > (size_t)G16_MAX_LAUNCH || a.n_pairs < 1 || a.n_pairs > PB_MAX_PAIRS || (!a.one && !a.out_gt)) return hipErrorInvalidDevice;
  if ((a.shared_mask >> a.n_pairs) || (a.shared_mask && (!a.prepared || ((uintptr_t)a.prepared & 3))) || a.item_stride < bn254::pb_item_len(a.n_pairs, a.shared_mask)) return hipErrorInvalidDevice;
  memset(a.ws, 0x5a, a.n * (size_t)G16_WS_BYTES_PER_PROOF);
  if (a.one) (void)a.one[12 * BN_NL - 1];
  const size_t shared = (size_t)__builtin_popcount(a.shared_mask);
  if (shared) (void)a.prepared[shared * PB_PREP_DWORDS - 1];                // the last dword a run kernel reads
  const bool records_ok = !shared || bn254::pb_records_ok(a.prepared, a.shared_mask);
  const size_t rec_len = bn254::pb_item_len(a.n_pairs, a.shared_mask);
  for (size_t i = 0; i < a.n; i++) {
    const uint8_t* rec = a.pairs + i * a.item_stride;
    (void)rec[rec_len - 1];                                                 // the last byte the loader reads
    uint8_t gt[384];
    uint8_t st;
    if (!records_ok) st = BN254_ST_MALFORMED;
    else if (i < REAL_ITEMS) st = shared ? bn254::pb_item_shared_on_host(rec, a.n_pairs, a.shared_mask, a.prepared, gt) : bn254::pb_item_on_host(rec, a.n_pairs, gt);
    else st = rec[0] == 0xEE ? BN254_ST_REJECT : BN254_ST_ACCEPT;
    if (i >= REAL_ITEMS) memset(gt, (int)(i & 0xff), sizeof gt);
    const bool reached = st == BN254_ST_ACCEPT || st == BN254_ST_REJECT;
    if (a.out_gt && reached) memcpy(a.out_gt + 384 * i, gt, 384);
    if (reached && !a.one) st = BN254_ST_ACCEPT;
    a.status[i] = st;
  }
  return hipSuccess;
}

static void put_be(uint8_t* o, const bn254::Fp& a) { fp_to_be(o, a); }
static std::vector<uint8_t> g1_bytes(bool neg) {
  std::vector<uint8_t> b(64);
  bn254::G1Aff g; g.x = bn254::fp_one(); g.y = bn254::fp_add(bn254::fp_one(), bn254::fp_one());
  if (neg) g = bn254::g1_neg(g);
  put_be(b.data(), g.x); put_be(b.data() + 32, g.y);
  return b;
}
static std::vector<uint8_t> g2_bytes() {
  std::vector<uint8_t> b(128);
  bn254::G2Aff g; g.x = bn254::fp2_from_limbs(BN_G2_GEN[0], BN_G2_GEN[1]); g.y = bn254::fp2_from_limbs(BN_G2_GEN[2], BN_G2_GEN[3]);
  put_be(b.data(), g.x.c1); put_be(b.data() + 32, g.x.c0); put_be(b.data() + 64, g.y.c1); put_be(b.data() + 96, g.y.c0);
  return b;
}

// n PACKED items of k positions under `mask` at `stride`; every G2 point, shared or not, is the generator (identity for position >= 2).  The first three are real:
// e(G1, G2) e(-G1, G2) = 1 padded with identities of G1: ACCEPT; the same with the sign dropped: REJECT; G1 off its curve: NOT_ON_CURVE.  The others are markers --
// every seventh one 0xEE (REJECT), else zero bytes (ACCEPT)
static std::vector<uint8_t> make_items(size_t n, size_t k, unsigned mask, size_t stride, std::vector<uint8_t>& want) {
  std::vector<uint8_t> buf(n * stride, 0);
  want.assign(n, BN254_ACCEPT);
  const std::vector<uint8_t> pos = g1_bytes(false), neg = g1_bytes(true), q = g2_bytes();
  for (size_t i = 0; i < n; i++) {
    uint8_t* r = buf.data() + i * stride;
    if (i < REAL_ITEMS) {
      uint8_t* p = r;
      for (size_t j = 0; j < k; j++) {
        if (j < 2) memcpy(p, (j == 0 || i == 1) ? pos.data() : neg.data(), 64);
        if (!((mask >> j) & 1)) { if (j < 2) memcpy(p + 64, q.data(), 128); p += 192; } else p += 64;
      }
      if (i == 2) r[63] ^= 1;
      want[i] = i == 2 ? BN254_ERR_NOT_ON_CURVE : (k >= 2 && i == 0) ? BN254_ACCEPT : BN254_REJECT;
    } else if (i % 7 == 3) { r[0] = 0xEE; want[i] = BN254_REJECT; }
  }
  return buf;
}
// the records of the shared positions of make_items: the generator at positions 0 and 1, the identity behind
static std::vector<uint8_t> make_records(size_t k, unsigned mask) {
  std::vector<uint8_t> recs, one(BN254_G2_PREPARED_LEN), zero(128, 0);
  const std::vector<uint8_t> q = g2_bytes();
  for (size_t j = 0; j < k; j++)
    if ((mask >> j) & 1) {
      uint8_t st = 0xEE;
      CHECK(bn254_g2_prepare(j < 2 ? q.data() : zero.data(), one.data(), &st) == BN254_OK && st == BN254_ACCEPT);
      recs.insert(recs.end(), one.begin(), one.end());
    }
  return recs;
}

int main() {
  g_fake_device_count = 48;
  // ---- bn254_g2_prepare: exactly BN254_G2_PREPARED_LEN bytes written, rejections write nothing
  {
    std::vector<uint8_t> q = g2_bytes(), out(BN254_G2_PREPARED_LEN, 0xEE);        // a heap block of exactly the record's size: ASan sees one byte too many
    uint8_t st = 0xEE;
    CHECK(bn254_g2_prepare(q.data(), out.data(), &st) == BN254_OK && st == BN254_ACCEPT);
    uint32_t h[4]; memcpy(h, out.data(), 16);
    CHECK(h[0] == PB_PREP_MAGIC && h[1] == PB_PREP_VERSION && h[2] == 0 && h[3] == 0);
    std::vector<uint8_t> bad = q, keep(BN254_G2_PREPARED_LEN, 0xEE); bad[127] ^= 1;
    CHECK(bn254_g2_prepare(bad.data(), keep.data(), &st) == BN254_OK && st == BN254_ERR_NOT_ON_CURVE);
    memset(bad.data(), 0xff, 32);
    CHECK(bn254_g2_prepare(bad.data(), keep.data(), &st) == BN254_OK && st == BN254_ERR_NOT_MEMBER);
    for (auto b : keep) CHECK(b == 0xEE);
    CHECK(bn254_g2_prepare(nullptr, keep.data(), &st) == BN254_E_BAD_ARG && bn254_g2_prepare(q.data(), nullptr, &st) == BN254_E_BAD_ARG && bn254_g2_prepare(q.data(), keep.data(), nullptr) == BN254_E_BAD_ARG);
  }
  // ---- the argument checks: BN254_E_BAD_ARG before a device is looked at (ordinal 99 does not exist), nothing written, no launch
  {
    const size_t k = 4; const unsigned mask = 0xE;
    std::vector<uint8_t> item(192 * 8), st(2, 0xEE), gt(768, 0xEE), recs = make_records(k, mask);
    const size_t packed = 192 + 3 * 64;
    auto clean = [&] { for (auto b : st) if (b != 0xEE) return false; for (auto b : gt) if (b != 0xEE) return false; return true; };
    CHECK(bn254_pairing_check_batch_shared(item.data(), packed, k, 0x10, recs.data(), 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_shared(item.data(), packed, k, mask, nullptr, 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_shared(item.data(), packed - 1, k, mask, recs.data(), 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_shared(nullptr, packed, k, mask, recs.data(), 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_shared(item.data(), SIZE_MAX / 2, k, mask, recs.data(), 3, st.data(), 99) == BN254_E_BAD_ARG && clean());
    { std::vector<uint8_t> bad = recs; bad[BN254_G2_PREPARED_LEN] ^= 1; CHECK(bn254_pairing_batch_shared(item.data(), packed, k, mask, bad.data(), 1, gt.data(), st.data(), 99) == BN254_E_BAD_ARG && clean()); }
    { std::vector<uint8_t> bad = recs; bad[2 * BN254_G2_PREPARED_LEN + 4] ^= 2; CHECK(bn254_pairing_check_batch_shared(item.data(), packed, k, mask, bad.data(), 1, st.data(), 99) == BN254_E_BAD_ARG && clean()); }
    CHECK(bn254_pairing_check_batch_shared_device(item.data(), packed, k, mask, recs.data() + 2, 1, st.data(), 99, nullptr) == BN254_E_BAD_ARG && clean());     // alignment
    CHECK(bn254_pairing_batch_shared(item.data(), packed, k, mask, recs.data(), 1, nullptr, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_batch_shared(item.data(), packed, k, mask, recs.data(), 0, nullptr, nullptr, 99) == BN254_OK && bn254_pairing_check_batch_shared(nullptr, packed, k, mask, recs.data(), 0, nullptr, 99) == BN254_OK);
    CHECK(bn254_pairing_check_batch_shared(item.data(), packed, k, mask, recs.data(), 1, st.data(), 99) == BN254_E_BAD_ARG && clean());      // past the argument checks: the device ordinal
    CHECK(bn254_dbg_pairing_batch_shared(item.data(), packed, k, mask, recs.data(), 1, gt.data(), st.data(), -1, 2) == BN254_E_BAD_ARG && clean());
    CHECK(g_pair_launches.load() == 0);
  }
  // ---- host calls of three passes at two masks, packed and padded items: the prepared records staged in front of every pass's items, no launch above the
  // reservation, every launch with the mask; then the GT entry
  for (auto shape : {std::pair<size_t, unsigned>{4, 0xEu}, std::pair<size_t, unsigned>{8, 0xAAu}, std::pair<size_t, unsigned>{2, 0x3u}}) {
    const size_t k = shape.first; const unsigned mask = shape.second;
    const size_t packed = bn254::pb_item_len((int)k, mask);
    const std::vector<uint8_t> recs = make_records(k, mask);
    for (size_t stride : {packed, packed + 9}) {
      const size_t pass = pb_host_pass_of(packed, recs.size(), 100000);
      CHECK(pass >= 64 && pass <= 1000);
      const size_t n = 2 * pass + 37;               // three passes
      std::vector<uint8_t> want, buf = make_items(n, k, mask, stride, want), st(n + 1, 0xEE), gt(384 * n + 1, 0xEE);
      const size_t before = g_pair_launches.load(), sbefore = g_shared_launches.load();
      CHECK(bn254_pairing_check_batch_shared(buf.data(), stride, k, mask, recs.data(), n, st.data(), 0) == 0 && st[n] == 0xEE);
      CHECK(g_pair_launches.load() - before == 3 && g_shared_launches.load() - sbefore == 3 && g_largest_launch.load() <= pass);
      for (size_t i = 0; i < pass; i++) CHECK(st[i] == want[i]);
      for (size_t i = pass + REAL_ITEMS; i < n; i++) if (i % pass >= REAL_ITEMS) CHECK(st[i] == want[i]);
      CHECK(bn254_pairing_batch_shared(buf.data(), stride, k, mask, recs.data(), n, gt.data(), st.data(), 0) == 0 && st[n] == 0xEE && gt[384 * n] == 0xEE);
      CHECK(st[0] == BN254_ACCEPT && st[1] == BN254_ACCEPT && st[2] == BN254_ERR_NOT_ON_CURVE && gt[384 * 5] == 5 && gt[384 * 5 + 383] == 5);
      CHECK(gt[31] == 1 && gt[32] == 0);              // item 0: 1 in GT from the host compile of the mixed run
    }
    // the probe's host compile equals the all-variable host compile on the expanded items (the first three)
    {
      std::vector<uint8_t> want, buf = make_items(3, k, mask, packed, want), st(3, 0xEE), gt(384 * 3, 0xEE);
      CHECK(bn254_dbg_pairing_batch_shared(buf.data(), packed, k, mask, recs.data(), 3, gt.data(), st.data(), -1, 0) == 0);
      for (size_t i = 0; i < 3; i++) CHECK(st[i] == want[i]);
    }
  }
  // ---- the device entry: a reservation, then calls at and above it on a stream of the caller's; a corrupted record makes every item MALFORMED
  {
    const size_t k = 4; const unsigned mask = 0xE; const size_t stride = 400;
    std::vector<uint8_t> recs = make_records(k, mask);
    CHECK(bn254_pairing_reserve(100, 1) == 0);
    hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    for (size_t n : {(size_t)1, (size_t)100, (size_t)250}) {
      std::vector<uint8_t> want, buf = make_items(n, k, mask, stride, want), st(n + 1, 0xEE);
      CHECK(bn254_pairing_check_batch_shared_device(buf.data(), stride, k, mask, recs.data(), n, st.data(), 1, s) == 0 && st[n] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    std::vector<uint8_t> bad = recs; bad[0] ^= 1;
    std::vector<uint8_t> want, buf = make_items(70, k, mask, stride, want), st(71, 0xEE);
    CHECK(bn254_pairing_check_batch_shared_device(buf.data(), stride, k, mask, bad.data(), 70, st.data(), 1, s) == 0 && st[70] == 0xEE);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == BN254_ERR_MALFORMED);
    // shared_mask 0 is the all-variable entry
    std::vector<uint8_t> item(192), st1(1, 0xEE);
    const size_t sbefore = g_shared_launches.load();
    CHECK(bn254_pairing_check_batch_shared_device(item.data(), 192, 1, 0, nullptr, 1, st1.data(), 1, s) == 0 && st1[0] == BN254_ACCEPT && g_shared_launches.load() == sbefore);
    hipStreamDestroy(s);
  }
  // ---- an allocation failure at every allocation of a call, each on a device of its own that has passed its self-test: an error code, nothing written, and the same
  // call repeated without the failure answers right (nothing stale, nothing freed twice; leak detection is on)
  {
    const size_t n = 20, k = 4; const unsigned mask = 0xE; const size_t stride = bn254::pb_item_len((int)k, mask);
    std::vector<uint8_t> want, buf = make_items(n, k, mask, stride, want), recs = make_records(k, mask);
    bool through = false;
    int dev = 2;
    for (size_t fail = 1; fail < 40 && !through; fail++, dev++) {
      unsigned m = 0; float ms = 0;
      CHECK(bn254_device_selftest(dev, &m, &ms) == 0);
      std::vector<uint8_t> st(n + 1, 0xEE), gt(384 * n + 1, 0xEE);
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      const int rc = bn254_pairing_batch_shared(buf.data(), stride, k, mask, recs.data(), n, gt.data(), st.data(), dev);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) through = true;
      else { CHECK(rc == BN254_E_HIP || rc == BN254_E_NOMEM); for (auto b : st) CHECK(b == 0xEE); }
      CHECK(bn254_pairing_check_batch_shared(buf.data(), stride, k, mask, recs.data(), n, st.data(), dev) == 0 && st[n] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    CHECK(through && dev > 6);
  }
  // ---- two host threads on one device, one through the host entry and one through the device entry, with different masks: the device's lock serialises them and
  // the staging (records and items) belongs to one call at a time
  {
    const int dev = 46;
    std::atomic<int> bad{0};
    auto worker = [&](int which) {
      const size_t k = which ? 2 : 8; const unsigned mask = which ? 0x3u : 0xAAu;
      const std::vector<uint8_t> recs = make_records(k, mask);
      const size_t stride = bn254::pb_item_len((int)k, mask) + 4;
      for (int it = 0; it < 12; it++) {
        const size_t n = 30 + 17 * (size_t)it + (size_t)which;
        std::vector<uint8_t> want, buf = make_items(n, k, mask, stride, want), st(n, 0xEE);
        const int rc = which ? bn254_pairing_check_batch_shared_device(buf.data(), stride, k, mask, recs.data(), n, st.data(), dev, nullptr)
                             : bn254_pairing_check_batch_shared(buf.data(), stride, k, mask, recs.data(), n, st.data(), dev);
        if (rc != 0 || st != want) bad++;
      }
    };
    std::thread t0(worker, 0), t1(worker, 1);
    t0.join(); t1.join();
    CHECK(bad.load() == 0);
  }
  printf("hostsan_pairing_shared: %zu stand-in launches of the pairing batch (%zu with shared positions), the largest of %zu items, %zu allocations still live (the per-device workspaces)\nhostsan_pairing_shared ok\n",
         g_pair_launches.load(), g_shared_launches.load(), g_largest_launch.load(), g_fake_live_allocs.load());
  return 0;
}
