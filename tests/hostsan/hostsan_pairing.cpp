// The batch pairing product (csrc/bn254_capi_pairing.hip: bn254_pairing_check_batch, _device, bn254_pairing_batch, bn254_pairing_reserve) under the sanitizers: the
// host half of the library as ONE translation unit with the stand-in HIP runtime of hostsan_main.cpp (whose main is set aside), plus the pairing file itself, which is
// not part of that unit.  In the place of bn254_launch_pairing_batch stands the host compile of the kernels' bodies (csrc/bn254_pairing_batch.h::pb_item_on_host) for
// the first items of every launch and a marker rule for the rest, on the host memory the stand-in runtime hands out -- so the extents of the records, the workspace,
// the status bytes and the GT values of every launch are checked by AddressSanitizer against what the host code allocated.
//   BN254_PAIRING_PASS=1000 hostsan_pairing        (the environment lowers the items per pass so that calls of a few thousand items make several)
#include "hip/hip_runtime.h"
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_pairing.hip"
#include <thread>

static std::atomic<size_t> g_pair_launches{0}, g_largest_launch{0};
#define REAL_ITEMS 3      // items per launch that go through the host compile of the kernels; the others: first byte 0xEE = REJECT, else ACCEPT
hipError_t bn254_launch_pairing_batch(const bn254::PairingLaunchArgs& a, hipStream_t) {
  g_launches++; g_pair_launches++;
  size_t seen = g_largest_launch.load();
  while (a.n > seen && !g_largest_launch.compare_exchange_weak(seen, a.n)) {}
  if (a.n == 0 || a.n > (size_t)G16_MAX_LAUNCH || a.n_pairs < 1 || a.n_pairs > PB_MAX_PAIRS || (!a.one && !a.out_gt)) return hipErrorInvalidDevice;
  memset(a.ws, 0x5a, a.n * (size_t)G16_WS_BYTES_PER_PROOF);              // the launch owns a workspace lane per item: ASan checks the extent
  if (a.one) (void)a.one[12 * BN_NL - 1];
  for (size_t i = 0; i < a.n; i++) {
    const uint8_t* rec = a.pairs + i * a.item_stride;
    (void)rec[(size_t)PB_PAIR_LEN * a.n_pairs - 1];                       // the last byte the loader reads
    uint8_t gt[384];
    uint8_t st = i < REAL_ITEMS ? bn254::pb_item_on_host(rec, a.n_pairs, gt) : (rec[0] == 0xEE ? BN254_ST_REJECT : BN254_ST_ACCEPT);
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
static std::vector<uint8_t> cat(std::initializer_list<std::vector<uint8_t>> parts) { std::vector<uint8_t> v; for (auto& p : parts) v.insert(v.end(), p.begin(), p.end()); return v; }

// n items of k pairs at `stride`: the first three real (e(G1, G2) e(-G1, G2) = 1 padded with identities: ACCEPT; the same with the sign dropped: REJECT; G1 off
// its curve: NOT_ON_CURVE), the others markers -- every seventh one 0xEE (REJECT), else zero bytes (ACCEPT)
static std::vector<uint8_t> make_items(size_t n, size_t k, size_t stride, std::vector<uint8_t>& want) {
  std::vector<uint8_t> buf(n * stride, 0);
  want.assign(n, BN254_ACCEPT);
  const std::vector<uint8_t> pos = cat({g1_bytes(false), g2_bytes()}), neg = cat({g1_bytes(true), g2_bytes()});
  for (size_t i = 0; i < n; i++) {
    uint8_t* r = buf.data() + i * stride;
    if (i < REAL_ITEMS) {
      memcpy(r, pos.data(), 192);
      if (k >= 2) memcpy(r + 192, i == 1 ? pos.data() : neg.data(), 192);
      if (i == 2) r[63] ^= 1;
      want[i] = i == 2 ? BN254_ERR_NOT_ON_CURVE : (k >= 2 && i == 0) ? BN254_ACCEPT : BN254_REJECT;
    } else if (i % 7 == 3) { r[0] = 0xEE; want[i] = BN254_REJECT; }
  }
  return buf;
}

int main() {
  g_fake_device_count = 48;
  uint64_t plan[4];
  // ---- the argument checks: BN254_E_BAD_ARG before a device is looked at (ordinal 99 does not exist), nothing written
  {
    std::vector<uint8_t> item(192 * 8), st(2, 0xEE), gt(768, 0xEE);
    auto clean = [&] { for (auto b : st) if (b != 0xEE) return false; for (auto b : gt) if (b != 0xEE) return false; return true; };
    CHECK(bn254_pairing_check_batch(nullptr, 192, 1, 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch(item.data(), 192, 1, 1, nullptr, 99) == BN254_E_BAD_ARG);
    CHECK(bn254_pairing_check_batch(item.data(), 192, 0, 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch(item.data(), 192 * 9, 9, 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch(item.data(), 383, 2, 1, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch(item.data(), SIZE_MAX / 2, 1, 3, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_device(item.data(), 191, 1, 1, st.data(), 99, nullptr) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_batch(item.data(), 192, 1, 1, nullptr, st.data(), 99) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_batch(item.data(), 192, 1, 0, nullptr, nullptr, 99) == BN254_OK && bn254_pairing_check_batch(nullptr, 192, 1, 0, nullptr, 99) == BN254_OK);
    CHECK(bn254_pairing_check_batch(item.data(), 192, 1, 1, st.data(), 99) == BN254_E_BAD_ARG && clean());       // past the argument checks: the device ordinal
    CHECK(bn254_dbg_pairing_plan(0, 1, plan) == BN254_E_BAD_ARG && bn254_dbg_pairing_plan(1, 1, nullptr) == BN254_E_BAD_ARG);
    CHECK(g_pair_launches.load() == 0);
  }
  // ---- the pass plan against the reservation: host calls of several passes at every pair count, packed and padded records; no launch above what was allocated
  for (size_t k : {1, 2, 3, 8}) {
    for (size_t stride : {192 * k, 192 * k + 9}) {
      CHECK(bn254_dbg_pairing_plan(k, 100000, plan) == 0);
      const size_t n = 2 * (size_t)plan[1] + 37;               // three passes
      CHECK(plan[1] >= 64 && plan[1] <= plan[0] && plan[2] >= 1);
      std::vector<uint8_t> want, buf = make_items(n, k, stride, want), st(n + 1, 0xEE), gt(384 * n + 1, 0xEE);
      const size_t before = g_pair_launches.load();
      CHECK(bn254_pairing_check_batch(buf.data(), stride, k, n, st.data(), 0) == 0 && st[n] == 0xEE);
      CHECK(g_pair_launches.load() - before == 3 && g_largest_launch.load() <= plan[1]);
      // every pass starts with the stand-in's real items: those of the first pass are the vectors, the later passes' first items are markers run through the loader
      for (size_t i = 0; i < (size_t)plan[1]; i++) CHECK(st[i] == want[i]);
      for (size_t i = plan[1] + REAL_ITEMS; i < n; i++) if (i % plan[1] >= REAL_ITEMS) CHECK(st[i] == want[i]);
      CHECK(bn254_pairing_batch(buf.data(), stride, k, n, gt.data(), st.data(), 0) == 0 && st[n] == 0xEE && gt[384 * n] == 0xEE);
      CHECK(st[0] == BN254_ACCEPT && st[1] == BN254_ACCEPT && st[2] == BN254_ERR_NOT_ON_CURVE && gt[384 * 5] == 5 && gt[384 * 5 + 383] == 5);
    }
  }
  // the device entry: a reservation, then calls at and above it (several launches against one workspace), on a stream of the caller's
  {
    CHECK(bn254_dbg_pairing_plan(2, 1, plan) == 0);
    CHECK(bn254_pairing_reserve(100, 1) == 0);
    hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    for (size_t n : {(size_t)1, (size_t)100, (size_t)250}) {
      std::vector<uint8_t> want, buf = make_items(n, 2, 400, want), st(n + 1, 0xEE);
      CHECK(bn254_pairing_check_batch_device(buf.data(), 400, 2, n, st.data(), 1, s) == 0 && st[n] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    CHECK(bn254_dbg_pairing_plan(2, 1 << 20, plan) == 0);
    const size_t n = 2 * (size_t)plan[0] + 5;
    std::vector<uint8_t> want, buf = make_items(n, 2, 384, want), st(n + 1, 0xEE);
    const size_t before = g_pair_launches.load();
    CHECK(bn254_pairing_check_batch_device(buf.data(), 384, 2, n, st.data(), 1, s) == 0 && st[n] == 0xEE);
    CHECK(g_pair_launches.load() - before == 3);
    hipStreamDestroy(s);
  }
  // ---- an allocation failure at every allocation of a call, each on a device of its own that has passed its self-test: an error code, nothing written beyond the
  // items, and the same call repeated without the failure answers right (nothing stale, nothing freed twice; leak detection is on)
  {
    const size_t n = 20, k = 3, stride = 192 * k;
    std::vector<uint8_t> want, buf = make_items(n, k, stride, want);
    bool through = false;
    int dev = 2;
    for (size_t fail = 1; fail < 40 && !through; fail++, dev++) {
      unsigned mask = 0; float ms = 0;
      CHECK(bn254_device_selftest(dev, &mask, &ms) == 0);
      std::vector<uint8_t> st(n + 1, 0xEE), gt(384 * n + 1, 0xEE);
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      const int rc = bn254_pairing_batch(buf.data(), stride, k, n, gt.data(), st.data(), dev);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) through = true;
      else { CHECK(rc == BN254_E_HIP || rc == BN254_E_NOMEM); for (auto b : st) CHECK(b == 0xEE); }
      CHECK(bn254_pairing_check_batch(buf.data(), stride, k, n, st.data(), dev) == 0 && st[n] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    CHECK(through && dev > 6);     // ended by a call that made every allocation (at least: 1 in GT, workspace, four staging buffers, two GT buffers)
  }
  // ---- two host threads on one device, one through the host entry and one through the device entry: the device's lock serialises them
  {
    const int dev = 46;
    std::atomic<int> bad{0};
    auto worker = [&](int which) {
      const size_t k = which ? 2 : 8;
      for (int it = 0; it < 12; it++) {
        const size_t n = 30 + 17 * (size_t)it + (size_t)which;
        std::vector<uint8_t> want, buf = make_items(n, k, 192 * k + 4, want), st(n, 0xEE);
        const int rc = which ? bn254_pairing_check_batch_device(buf.data(), 192 * k + 4, k, n, st.data(), dev, nullptr)
                             : bn254_pairing_check_batch(buf.data(), 192 * k + 4, k, n, st.data(), dev);
        if (rc != 0 || st != want) bad++;
      }
    };
    std::thread t0(worker, 0), t1(worker, 1);
    t0.join(); t1.join();
    CHECK(bad.load() == 0);
  }
  printf("hostsan_pairing: %zu stand-in launches of the pairing batch, the largest of %zu items, %zu allocations still live (the per-device workspaces)\nhostsan_pairing ok\n",
         g_pair_launches.load(), g_largest_launch.load(), g_fake_live_allocs.load());
  return 0;
}
