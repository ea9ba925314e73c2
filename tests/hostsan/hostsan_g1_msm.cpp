// The entries of the G1 multi-scalar multiplication (csrc/bn254_capi_g1msm.hip: bn254_g1_bases_prepare, _free, _count, bn254_g1_msm_batch, _device,
// bn254_g1_msm_reserve; the probe bn254_dbg_g1_msm_batch) under the sanitizers, in the pattern of hostsan_kzg_fold.cpp: the host half of the library as ONE translation
// unit with the stand-in HIP runtime of hostsan_main.cpp (whose main is set aside) plus the pairing file (for the host stream the host entry borrows) and the G1 MSM file.  In the place of the launchers stand: for k_g1_msm_load the host
// compile of the loader (csrc/bn254_g1msm.h::g1msm_load_item -- the checks, the scalars, the term records) for the first items of every launch and a marker rule for
// the rest; for k_g1_msm_store the host compile of the store (g1msm_store_item) for every item -- on the memory the stand-in runtime hands out, so the extents of the
// staged items (item lengths padded to whole dwords, strides that are no multiple of 4), the term records, rows, scratch, the sums' words and the 65 result bytes per
// item of every launch are checked by AddressSanitizer against what the host code allocated and copied.  (The stand-in walk of hostsan_main.cpp leaves the sum (0, 0).)
//   BN254_G1_MSM_PASS=1000 hostsan_g1_msm
#include "hip/hip_runtime.h"
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_pairing.hip"
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_g1msm.hip"
#include <thread>

static std::atomic<size_t> g_load_launches{0}, g_store_launches{0}, g_largest_launch{0};
hipError_t bn254_launch_pairing_batch(const bn254::PairingLaunchArgs&, hipStream_t) { return hipErrorInvalidDevice; }      // the pairing file is here for its host stream alone
#define REAL_ITEMS 3      // items per launch that go through the host compile of the loader; the others: first byte 0xEE = "a point off its curve", else pending
hipError_t bn254_launch_g1msm_load(const bn254::G1MsmLoadArgs& a, hipStream_t) {
  g_launches++; g_load_launches++;
  size_t seen = g_largest_launch.load();
  while (a.n > seen && !g_largest_launch.compare_exchange_weak(seen, a.n)) {}
  if (a.n == 0 || a.n > G1MSM_MAX_PASS || !bn254::g1msm_shape_ok((size_t)a.n_var, (size_t)a.n_unit, (size_t)a.n_shared) || !a.items) return hipErrorInvalidDevice;
  const size_t len = G1MSM_ITEM_LEN(a.n_var, a.n_unit, a.n_shared);
  if (a.stride < len) return hipErrorInvalidDevice;
  const int n_terms = a.n_var + a.n_unit + a.n_shared;
  memset(a.terms, 0x21, a.n * (size_t)n_terms * MSM_TERM_DWORDS * sizeof(int32_t));
  memset(a.flags, 0x22, a.n * (size_t)n_terms);
  memset(a.status, 0x23, a.n);
  const bool aligned = ((((uintptr_t)a.items) | a.stride) & 3) == 0;      // the kernel's rule: dword loads of the item then
  for (size_t i = 0; i < a.n; i++) {
    const uint8_t* rec = a.items + i * a.stride;
    (void)rec[len - 1];                                                    // the last byte the loader reads
    if (i < REAL_ITEMS)
      a.status[i] = (uint8_t)bn254::g1msm_load_item(rec, aligned, a.n_var, a.n_unit, a.n_shared, a.dead_bases, a.strict, a.terms + i * (size_t)n_terms * MSM_TERM_DWORDS,
                                                     a.flags + i * (size_t)n_terms);
    else a.status[i] = rec[0] == 0xEE ? (uint8_t)BN254_ST_NOT_ON_CURVE : (uint8_t)BN254_ST_PENDING;
  }
  return hipSuccess;
}
hipError_t bn254_launch_g1msm_store(const uint32_t* words, const uint8_t* inf, const uint8_t* st, size_t n, uint8_t* out, uint8_t* status, hipStream_t) {
  g_launches++; g_store_launches++;
  if (n == 0 || n > G1MSM_MAX_PASS || ((uintptr_t)words & 15)) return hipErrorInvalidDevice;
  for (size_t i = 0; i < n; i++) bn254::g1msm_store_item(out + 64 * i, status + i, st[i], words + 16 * i, inf[i] != 0, (((uintptr_t)out) & 3) == 0);
  return hipSuccess;
}

static std::vector<uint8_t> g1_bytes() {
  std::vector<uint8_t> b(64);
  bn254::G1Aff g; g.x = bn254::fp_one(); g.y = bn254::fp_add(bn254::fp_one(), bn254::fp_one());
  fp_to_be(b.data(), g.x); fp_to_be(b.data() + 32, g.y);
  return b;
}
struct Shape { size_t v, u, s; size_t len() const { return BN254_G1_MSM_ITEM_LEN(v, u, s); } };
// n items of a shape at `stride`, in a heap block that ends with the LAST ITEM (not with its stride): a read past an item's end is seen.  The first three are real:
// every point G1 and small scalars (summed), the last point off its curve (NOT_ON_CURVE; a shape without points: summed), the first scalar 2^256 - 1 (summed; strict:
// NOT_MEMBER; a shape without scalars: summed).  The others are markers: `bad(i)` items start with 0xEE.  want: the status bytes
static std::vector<uint8_t> make_items(size_t n, size_t stride, const Shape& sh, const std::function<bool(size_t)>& bad, bool strict, std::vector<uint8_t>& want) {
  const size_t len = sh.len();
  std::vector<uint8_t> buf((n - 1) * stride + len, 0);
  want.assign(n, BN254_ACCEPT);
  const std::vector<uint8_t> p = g1_bytes();
  for (size_t i = 0; i < n; i++) {
    uint8_t* r = buf.data() + i * stride;
    if (i < REAL_ITEMS) {
      for (size_t t = 0; t < sh.v; t++) { memcpy(r + 96 * t, p.data(), 64); r[96 * t + 95] = (uint8_t)(t + 2); }
      for (size_t t = 0; t < sh.u; t++) memcpy(r + 96 * sh.v + 64 * t, p.data(), 64);
      for (size_t t = 0; t < sh.s; t++) r[96 * sh.v + 64 * sh.u + 32 * t + 31] = (uint8_t)(t + 1);
      if (i == 1 && sh.v + sh.u) { r[(sh.u ? 96 * sh.v + 64 * (sh.u - 1) : 96 * (sh.v - 1)) + 63] ^= 1; want[i] = BN254_ERR_NOT_ON_CURVE; }
      if (i == 2 && sh.v + sh.s) { memset(r + (sh.v ? 64 : 64 * sh.u), 0xff, 32); if (strict) want[i] = BN254_ERR_NOT_MEMBER; }
    } else if (bad(i)) { r[0] = 0xEE; want[i] = BN254_ERR_NOT_ON_CURVE; }
  }
  return buf;
}
static void* make_bases(size_t count, int device) {
  std::vector<uint8_t> pts;
  const std::vector<uint8_t> p = g1_bytes();
  for (size_t j = 0; j < count; j++) { if (count > 1 && j == 1) pts.insert(pts.end(), 64, 0); else pts.insert(pts.end(), p.begin(), p.end()); }      // one identity base
  void* h = nullptr; uint8_t st = 0xEE;
  CHECK(bn254_g1_bases_prepare(pts.data(), count, device, &h, &st) == BN254_OK && st == BN254_ACCEPT && h && bn254_g1_bases_count(h) == count);
  return h;
}
static bool all_zero(const std::vector<uint8_t>& v, size_t n) { for (size_t i = 0; i < n; i++) if (v[i]) return false; return true; }

int main() {
  g_fake_device_count = 48;
  const auto never = [](size_t) { return false; };
  const std::vector<uint8_t> gen = g1_bytes();
  // ---- the argument checks: BN254_E_BAD_ARG before a device is looked at (ordinal 99 does not exist), nothing written, no launch
  {
    std::vector<uint8_t> item(96 * 4), out(64 * 4, 0xEE), st(4, 0xEE);
    auto clean = [&] { for (auto b : st) if (b != 0xEE) return false; for (auto b : out) if (b != 0xEE) return false; return true; };
    CHECK(bn254_g1_msm_batch(nullptr, 96, 1, 0, 0, nullptr, 4, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 96, 1, 0, 0, nullptr, 4, nullptr, st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 96, 1, 0, 0, nullptr, 4, out.data(), nullptr, 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 95, 1, 0, 0, nullptr, 4, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 96, 0, 0, 0, nullptr, 4, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 4096, 17, 0, 0, nullptr, 1, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 4096, 0, 5, 0, nullptr, 1, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 4096, 0, 0, 17, nullptr, 1, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch(item.data(), 96, 0, 0, 1, nullptr, 4, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());      // shared terms, no handle
    CHECK(bn254_g1_msm_batch(item.data(), 96, 1, 0, 0, nullptr, 4, out.data(), st.data(), 99, BN254_FLAG_RLC) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch_device(item.data(), 96, 1, 0, 0, nullptr, 4, out.data(), nullptr, 99, nullptr, 0) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_batch_device(item.data(), 96, 1, 0, 0, nullptr, 4, out.data(), st.data(), 99, nullptr, 16) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_g1_msm_reserve(10, 0, 0, 0, 99) == BN254_E_BAD_ARG && bn254_g1_msm_reserve(10, 17, 0, 0, 99) == BN254_E_BAD_ARG);
    CHECK(bn254_g1_msm_batch(nullptr, 96, 1, 0, 0, nullptr, 0, nullptr, nullptr, 99, 0) == BN254_OK);
    void* h = nullptr; uint8_t bst = 0xEE;
    CHECK(bn254_g1_bases_prepare(nullptr, 1, 99, &h, &bst) == BN254_E_BAD_ARG && bn254_g1_bases_prepare(gen.data(), 0, 99, &h, &bst) == BN254_E_BAD_ARG && bst == 0xEE && !h);
    CHECK(bn254_g1_bases_prepare(gen.data(), 17, 99, &h, &bst) == BN254_E_BAD_ARG && bn254_g1_bases_prepare(gen.data(), 1, 99, nullptr, &bst) == BN254_E_BAD_ARG);
    std::vector<uint8_t> off = gen; off[63] ^= 1;
    CHECK(bn254_g1_bases_prepare(off.data(), 1, 99, &h, &bst) == BN254_OK && bst == BN254_ERR_NOT_ON_CURVE && !h);      // decided before the device is looked at
    CHECK(bn254_g1_bases_count(nullptr) == 0);
    bn254_g1_bases_free(nullptr);
    CHECK(bn254_g1_msm_batch(item.data(), 96, 1, 0, 0, nullptr, 4, out.data(), st.data(), 99, 0) == BN254_E_BAD_ARG && clean());      // past the argument checks: the device ordinal
    CHECK(g_load_launches.load() == 0);
  }
  // ---- handles: prepare, count, use, the limits of a handle, the wrong device, free
  {
    void* a = make_bases(16, 0);
    void* b = make_bases(2, 1);
    const Shape sh{1, 1, 2};
    std::vector<uint8_t> want, buf = make_items(70, sh.len(), sh, never, false, want), out(64 * 70 + 1, 0xEE), st(71, 0xEE);
    CHECK(bn254_g1_msm_batch(buf.data(), sh.len(), 1, 1, 3, b, 70, out.data(), st.data(), 1, 0) == BN254_E_BAD_ARG);      // n_shared above the handle's count
    CHECK(bn254_g1_msm_batch(buf.data(), sh.len(), 1, 1, 2, b, 70, out.data(), st.data(), 0, 0) == BN254_E_BAD_ARG);      // device 0, the handle is device 1's
    CHECK(bn254_g1_msm_batch(buf.data(), sh.len(), 1, 1, 2, out.data(), 70, out.data(), st.data(), 0, 0) == BN254_E_BAD_ARG);      // no handle of this library
    CHECK(st[0] == 0xEE && out[0] == 0xEE);
    CHECK(bn254_g1_msm_batch(buf.data(), sh.len(), 1, 1, 2, b, 70, out.data(), st.data(), 1, 0) == 0 && st[70] == 0xEE && out[64 * 70] == 0xEE);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == want[i]);
    CHECK(bn254_g1_msm_batch(buf.data(), sh.len(), 1, 1, 2, a, 70, out.data(), st.data(), 0, 0) == 0);
    bn254_g1_bases_free(a);
    CHECK(bn254_g1_msm_batch(buf.data(), sh.len(), 1, 1, 2, b, 70, out.data(), st.data(), 1, 0) == 0);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == want[i]);
    bn254_g1_bases_free(b);
  }
  // ---- host calls of three passes (BN254_G1_MSM_PASS=1000), packed and padded items, exact and strict: no launch above a pass, out and status of every pass in place
  {
    void* bases = make_bases(16, 0);
    for (const Shape& sh : {Shape{1, 0, 0}, Shape{0, 2, 0}, Shape{3, 1, 2}, Shape{0, 0, 1}, Shape{16, 4, 16}})
      for (size_t pad : {(size_t)0, (size_t)9})
        for (unsigned flags : {0u, (unsigned)BN254_FLAG_STRICT_SCALARS}) {
          const size_t pass = 1000, n = 2 * pass + 37, stride = sh.len() + pad;
          std::vector<uint8_t> want, buf = make_items(n, stride, sh, [](size_t i) { return i % 7 == 3; }, flags != 0, want), st(n + 1, 0xEE), out(64 * n + 1, 0xEE);
          const size_t before = g_load_launches.load(), sbefore = g_store_launches.load();
          CHECK(bn254_g1_msm_batch(buf.data(), stride, sh.v, sh.u, sh.s, sh.s ? bases : nullptr, n, out.data(), st.data(), 0, flags) == 0 && st[n] == 0xEE && out[64 * n] == 0xEE);
          CHECK(g_load_launches.load() - before == 3 && g_store_launches.load() - sbefore == 3 && g_largest_launch.load() <= pass);
          for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
          CHECK(all_zero(out, 64 * n));      // the stand-in walk sums to (0, 0); a decided item leaves zero bytes
        }
    bn254_g1_bases_free(bases);
  }
  // the probe's host compile on the real items: the loader's statuses and the sums, nothing written past the buffers
  for (const Shape& sh : {Shape{1, 0, 0}, Shape{2, 1, 3}, Shape{0, 2, 0}}) {
    std::vector<uint8_t> want, buf = make_items(3, sh.len() + 1, sh, never, true, want), st(4, 0xEE), out(64 * 3 + 1, 0xEE), pts;
    for (size_t j = 0; j < sh.s; j++) pts.insert(pts.end(), gen.begin(), gen.end());
    int info[6];
    for (int joint : {0, 2})
      for (size_t budget : {(size_t)0, (size_t)64}) {
        CHECK(bn254_dbg_g1_msm_batch(buf.data(), sh.len() + 1, sh.v, sh.u, sh.s, sh.s ? pts.data() : nullptr, sh.s, 3, BN254_FLAG_STRICT_SCALARS, budget, joint, out.data(), st.data(), info, -1) == 0);
        CHECK(st[0] == want[0] && st[1] == want[1] && st[2] == want[2] && st[3] == 0xEE && out[64 * 3] == 0xEE && info[0] >= 1 && info[0] <= 32);
        bool any = false, none = true;
        for (int q = 0; q < 64; q++) { any |= out[q] != 0; none &= out[64 + q] == 0; }
        CHECK(any && none);      // item 0 is summed to a point; item 1 is decided: zero bytes
      }
    CHECK(bn254_dbg_g1_msm_batch(buf.data(), sh.len() + 1, sh.v, sh.u, sh.s + 1, pts.data(), sh.s, 3, 0, 0, 0, out.data(), st.data(), info, -1) == BN254_E_BAD_ARG);
  }
  // ---- the device entry: a reservation, then calls at and above it on a stream of the caller's -- at or below the reservation NOTHING is allocated
  {
    const int dev = 2;
    void* bases = make_bases(3, dev);
    for (const Shape& sh : {Shape{2, 1, 3}, Shape{16, 0, 0}}) {
      const size_t stride = sh.len() + 2;
      CHECK(bn254_g1_msm_reserve(100, sh.v, sh.u, sh.s, dev) == 0);
      hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
      for (size_t n : {(size_t)1, (size_t)100, (size_t)250, (size_t)2300}) {
        std::vector<uint8_t> want, buf = make_items(n, stride, sh, [](size_t i) { return i % 5 == 4; }, false, want), st(n + 1, 0xEE), out(64 * n + 2, 0xEE);
        const size_t live = g_fake_live_allocs.load();
        CHECK(bn254_g1_msm_batch_device(buf.data(), stride, sh.v, sh.u, sh.s, sh.s ? bases : nullptr, n, out.data() + 1, st.data(), dev, s, 0) == 0 && st[n] == 0xEE);
        CHECK(out[0] == 0xEE && out[64 * n + 1] == 0xEE);      // an odd address: the store's byte path
        CHECK(n > 100 || g_fake_live_allocs.load() == live);
        for (size_t i = 0; i < n; i++) if (i < REAL_ITEMS || i % 1000 >= REAL_ITEMS) CHECK(st[i] == want[i]);
      }
      hipStreamDestroy(s);
    }
    bn254_g1_bases_free(bases);
  }
  // ---- an allocation failure at every allocation of a call, each on a device of its own that has passed its self-test: BN254_E_NOMEM, nothing written, and the same
  // call repeated without the failure answers right (nothing stale, nothing freed twice; leak detection is on).  First the handle, then the batch
  {
    bool through = false;
    int dev = 4;
    for (size_t fail = 1; fail < 20 && !through; fail++, dev++) {
      unsigned m = 0; float ms = 0;
      CHECK(bn254_device_selftest(dev, &m, &ms) == 0);
      std::vector<uint8_t> pts;
      for (int j = 0; j < 3; j++) pts.insert(pts.end(), gen.begin(), gen.end());
      void* h = nullptr; uint8_t bst = 0xEE;
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      const int rc = bn254_g1_bases_prepare(pts.data(), 3, dev, &h, &bst);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) { through = true; CHECK(h && bst == BN254_ACCEPT); bn254_g1_bases_free(h); }
      else CHECK(rc == BN254_E_NOMEM && !h);
      CHECK(bn254_g1_bases_prepare(pts.data(), 3, dev, &h, &bst) == 0 && h && bn254_g1_bases_count(h) == 3);
      bn254_g1_bases_free(h);
    }
    CHECK(through && dev > 4 + 3);
  }
  {
    const Shape sh{16, 4, 16};
    const size_t n = 70;
    std::vector<uint8_t> want, buf = make_items(n, sh.len(), sh, [](size_t i) { return i == 9; }, false, want);
    bool through = false;
    int dev = 24;
    for (size_t fail = 1; fail < 30 && !through; fail++, dev++) {
      unsigned m = 0; float ms = 0;
      CHECK(bn254_device_selftest(dev, &m, &ms) == 0);
      void* bases = make_bases(16, dev);
      std::vector<uint8_t> st(n + 1, 0xEE), out(64 * n + 1, 0xEE);
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      const int rc = bn254_g1_msm_batch(buf.data(), sh.len(), sh.v, sh.u, sh.s, bases, n, out.data(), st.data(), dev, 0);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) through = true;
      else { CHECK(rc == BN254_E_NOMEM); for (auto b : st) CHECK(b == 0xEE); for (auto b : out) CHECK(b == 0xEE); }
      CHECK(bn254_g1_msm_batch(buf.data(), sh.len(), sh.v, sh.u, sh.s, bases, n, out.data(), st.data(), dev, 0) == 0 && st[n] == 0xEE && out[64 * n] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
      bn254_g1_bases_free(bases);
    }
    CHECK(through && dev > 24 + 8);
  }
  // ---- two host threads on one device with different shapes, one through the host entry and one through the device entry: the device's lock serialises them and
  // the staging and the term records belong to one call at a time
  {
    const int dev = 46;
    void* bases = make_bases(4, dev);
    std::atomic<int> bad{0};
    auto worker = [&](int which) {
      const Shape sh = which ? Shape{16, 0, 4} : Shape{0, 2, 0};
      const size_t stride = sh.len() + (which ? 0 : 5);
      for (int it = 0; it < 12; it++) {
        const size_t n = 30 + 170 * (size_t)it + (size_t)which;
        std::vector<uint8_t> want, buf = make_items(n, stride, sh, [&](size_t i) { return (i + (size_t)which) % 4 == 0; }, false, want), st(n, 0xEE), out(64 * n, 0xEE);
        const int rc = which ? bn254_g1_msm_batch_device(buf.data(), stride, sh.v, sh.u, sh.s, bases, n, out.data(), st.data(), dev, nullptr, 0)
                             : bn254_g1_msm_batch(buf.data(), stride, sh.v, sh.u, sh.s, nullptr, n, out.data(), st.data(), dev, 0);
        bool ok = rc == 0 && all_zero(out, 64 * n);
        for (size_t i = 0; i < n && ok; i++) if (i < REAL_ITEMS || i % 1000 >= REAL_ITEMS) ok = st[i] == want[i];
        if (!ok) bad++;
      }
    };
    std::thread t0(worker, 0), t1(worker, 1);
    t0.join(); t1.join();
    CHECK(bad.load() == 0);
    bn254_g1_bases_free(bases);
  }
  printf("hostsan_g1_msm: %zu stand-in launches of the loader, %zu of the store, the largest of %zu items, %zu allocations still live (the per-device buffers)\nhostsan_g1_msm ok\n",
         g_load_launches.load(), g_store_launches.load(), g_largest_launch.load(), g_fake_live_allocs.load());
  return 0;
}
