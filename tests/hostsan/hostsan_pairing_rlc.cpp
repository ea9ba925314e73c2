// BN254_FLAG_RLC on the pairing batch (csrc/bn254_capi_pairing_rlc.hip: bn254_pairing_check_batch_flags, _device, bn254_set_pairing_rlc_params, bn254_pairing_rlc_params,
// bn254_pairing_rlc_state, bn254_dbg_pairing_batch_rlc) under the sanitizers, in the pattern of hostsan_pairing_shared.cpp: the host half of the library as ONE
// translation unit with the stand-in HIP runtime of hostsan_main.cpp (whose main is set aside) plus the two pairing files.  In the place of the launchers stand marker
// rules on the memory the stand-in runtime hands out -- so the extents of the packed items, of the STAGED records and weights, of the item and group workspaces and of
// every status buffer of every launch are checked by AddressSanitizer against what the host code allocated and copied -- and the BN_HD bodies of the new kernels
// (pb_rlc_weigh_item, vm_miller_run_sub, the group sums, product and check) run for real through the probe's host compile on a small batch.
//   BN254_PAIRING_PASS=1000 hostsan_pairing_rlc
#include "hip/hip_runtime.h"
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_pairing.hip"
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_pairing_rlc.hip"
#include <thread>

static std::atomic<size_t> g_pair_launches{0}, g_joint_launches{0}, g_largest_launch{0};
// The stand-in of the pairing batch.  The loader marks an item by its first byte in dword i of the workspace (0xEE: the item is invalid), so that a launch behind the
// loader -- which reads no item -- still knows the verdict; a pending item ends REJECT with the mark, else ACCEPT.  A foreign record: every item MALFORMED.
hipError_t bn254_launch_pairing_batch(const bn254::PairingLaunchArgs& a, hipStream_t) {
  g_launches++; g_pair_launches++;
  size_t seen = g_largest_launch.load();
  while (a.n > seen && !g_largest_launch.compare_exchange_weak(seen, a.n)) {}
  if (a.n == 0 || a.n > (size_t)G16_MAX_LAUNCH || a.n_pairs < 1 || a.n_pairs > PB_MAX_PAIRS || (!a.one && !a.out_gt)) return hipErrorInvalidDevice;
  if ((a.shared_mask >> a.n_pairs) || (a.shared_mask && (!a.prepared || ((uintptr_t)a.prepared & 3)))) return hipErrorInvalidDevice;
  if (!a.skip_load && a.item_stride < bn254::pb_item_len(a.n_pairs, a.shared_mask)) return hipErrorInvalidDevice;
  const size_t shared = (size_t)__builtin_popcount(a.shared_mask);
  if (shared) (void)a.prepared[shared * PB_PREP_DWORDS - 1];
  (void)((volatile uint8_t*)a.ws)[a.n * (size_t)G16_WS_BYTES_PER_PROOF - 1];      // the last byte of the workspace of n items
  if (!a.skip_load) {
    memset(a.ws, 0, a.n * (size_t)G16_WS_BYTES_PER_PROOF);
    const bool ok = !shared || bn254::pb_records_ok(a.prepared, a.shared_mask);
    const size_t rec_len = bn254::pb_item_len(a.n_pairs, a.shared_mask);
    for (size_t i = 0; i < a.n; i++) {
      const uint8_t* rec = a.pairs + i * a.item_stride;
      (void)rec[rec_len - 1];
      a.ws[i] = rec[0] == 0xEE;
      a.status[i] = ok ? BN254_ST_PENDING : BN254_ST_MALFORMED;
    }
  }
  if (a.load_only || a.miller_only) return hipSuccess;
  (void)a.one[12 * BN_NL - 1];
  for (size_t i = 0; i < a.n; i++) {
    if (!(a.status[i] & BN254_ST_PENDING)) continue;
    if (a.out_gt) memset(a.out_gt + 384 * i, (int)(i & 0xff), 384);
    a.status[i] = a.ws[i] ? BN254_ST_REJECT : BN254_ST_ACCEPT;
  }
  return hipSuccess;
}
// The stand-in of everything between the loader and the scatter: the extents of the group buffers and of the weights; a group with a pending item is pending-then-decided
// (the scatter of hostsan_main.cpp fails group g of a launch when g % 16 == 3, whatever its byte), one without is ACCEPT
hipError_t bn254_launch_pairing_rlc_joint(const bn254::PairingRlcArgs& a, hipStream_t) {
  g_launches++; g_joint_launches++;
  if (a.n == 0 || !a.ws || !a.status || !a.grp_ws || !a.grp_status || !a.one) return hipErrorInvalidDevice;
  if (a.grp_form != bn254::PAIRING_FORM_LANES && a.grp_form != bn254::PAIRING_FORM_COOP) return hipErrorInvalidDevice;
  const size_t groups = (a.n + 63) / 64;
  memset(a.grp_ws, 0x5a, groups * (size_t)G16_WS_BYTES_PER_PROOF);
  if (a.weights) (void)a.weights[4 * a.n - 1];
  for (size_t g = 0; g < groups; g++) {
    bool any = false, bad = false;
    for (size_t i = 64 * g; i < 64 * g + 64 && i < a.n; i++)
      if (a.status[i] & BN254_ST_PENDING) { any = true; bad |= a.ws[i] != 0; }
    a.grp_status[g] = !any || !bad ? BN254_ST_ACCEPT : BN254_ST_REJECT;
    if (a.out_grp_gt) memset(a.out_grp_gt + 384 * g, (int)(g & 0xff), 384);
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
// the records of the shared positions: the generator at positions 0 and 1, the identity behind
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
// n REAL packed items of k positions (every G2 point the generator, identities from position 2 on): item i is e(G1, G2) e(-G1, G2) = 1 (ACCEPT), except i % 5 == 1: the
// sign dropped (REJECT) and i % 5 == 2: G1 off its curve
static std::vector<uint8_t> real_items(size_t n, size_t k, unsigned mask, std::vector<uint8_t>& want) {
  const size_t stride = bn254::pb_item_len((int)k, mask);
  std::vector<uint8_t> buf(n * stride, 0);
  want.assign(n, BN254_ACCEPT);
  const std::vector<uint8_t> pos = g1_bytes(false), neg = g1_bytes(true), q = g2_bytes();
  for (size_t i = 0; i < n; i++) {
    uint8_t *r = buf.data() + i * stride, *p = r;
    for (size_t j = 0; j < k; j++) {
      if (j < 2) memcpy(p, (j == 0 || i % 5 == 1) ? pos.data() : neg.data(), 64);
      if (!((mask >> j) & 1)) { if (j < 2) memcpy(p + 64, q.data(), 128); p += 192; } else p += 64;
    }
    if (i % 5 == 2) r[63] ^= 1;
    want[i] = i % 5 == 2 ? BN254_ERR_NOT_ON_CURVE : (k >= 2 && i % 5 != 1) ? BN254_ACCEPT : BN254_REJECT;
  }
  return buf;
}
// n MARKER items at `stride` for launches of `launch` items: the invalid ones (first byte 0xEE) sit in the groups the stand-in scatter fails (group g of a launch with
// g % 16 == 3), so that the exact check behind the synchronisation is what rejects them
static std::vector<uint8_t> marker_items(size_t n, size_t stride, size_t launch, std::vector<uint8_t>& want) {
  std::vector<uint8_t> buf(n * stride, 0);
  want.assign(n, BN254_ACCEPT);
  for (size_t i = 0; i < n; i++) {
    const size_t li = i % launch;
    if ((li / 64) % 16 == 3 && li % 7 == 3) { buf[i * stride] = 0xEE; want[i] = BN254_REJECT; }
  }
  return buf;
}

int main() {
  g_fake_device_count = 48;
  uint64_t s0[4], s1[4];
  CHECK(bn254_dbg_set_pairing_rlc_max_var(8) == 0);      // the default honours shapes without a variable position only; the harness drives every shape
  // ---- the knob: clamped below at 64, a negative value leaves it alone; null pointers
  {
    long was[1], now[1];
    CHECK(bn254_pairing_rlc_params(was) == 0 && was[0] >= 64);
    bn254_set_pairing_rlc_params(-5); CHECK(bn254_pairing_rlc_params(now) == 0 && now[0] == was[0]);
    bn254_set_pairing_rlc_params(0); CHECK(bn254_pairing_rlc_params(now) == 0 && now[0] == 64);
    bn254_set_pairing_rlc_params(100000); CHECK(bn254_pairing_rlc_params(now) == 0 && now[0] == 100000);
    CHECK(bn254_pairing_rlc_params(nullptr) == BN254_E_BAD_ARG && bn254_pairing_rlc_state(nullptr) == BN254_E_BAD_ARG);
    bn254_set_pairing_rlc_params(64);
  }
  // ---- the argument checks: BN254_E_BAD_ARG before a device is looked at (ordinal 99 does not exist), nothing written, no launch
  {
    const size_t k = 4; const unsigned mask = 0xE;
    std::vector<uint8_t> item(192 * 8), st(2, 0xEE), recs = make_records(k, mask);
    const size_t packed = 192 + 3 * 64;
    auto clean = [&] { for (auto b : st) if (b != 0xEE) return false; return true; };
    for (unsigned flags : {2u, 4u, (unsigned)BN254_FLAG_RLC | 2u, 0x80000000u}) {
      if (!(flags & ~(unsigned)BN254_FLAG_RLC)) continue;
      CHECK(bn254_pairing_check_batch_flags(item.data(), packed, k, mask, recs.data(), 1, st.data(), 99, flags) == BN254_E_BAD_ARG && clean());
      CHECK(bn254_pairing_check_batch_flags_device(item.data(), packed, k, mask, recs.data(), 1, st.data(), 99, nullptr, flags) == BN254_E_BAD_ARG && clean());
    }
    const unsigned F = BN254_FLAG_RLC;
    CHECK(bn254_pairing_check_batch_flags(item.data(), packed, k, 0x10, recs.data(), 1, st.data(), 99, F) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_flags(item.data(), packed, k, mask, nullptr, 1, st.data(), 99, F) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_flags(item.data(), packed - 1, k, mask, recs.data(), 1, st.data(), 99, F) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_flags(nullptr, packed, k, mask, recs.data(), 1, st.data(), 99, F) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_flags(item.data(), SIZE_MAX / 2, k, mask, recs.data(), 3, st.data(), 99, F) == BN254_E_BAD_ARG && clean());
    CHECK(bn254_pairing_check_batch_flags(item.data(), packed, 9, 0, nullptr, 1, st.data(), 99, F) == BN254_E_BAD_ARG && clean());
    { std::vector<uint8_t> bad = recs; bad[BN254_G2_PREPARED_LEN] ^= 1; CHECK(bn254_pairing_check_batch_flags(item.data(), packed, k, mask, bad.data(), 1, st.data(), 99, F) == BN254_E_BAD_ARG && clean()); }
    CHECK(bn254_pairing_check_batch_flags_device(item.data(), packed, k, mask, recs.data() + 2, 1, st.data(), 99, nullptr, F) == BN254_E_BAD_ARG && clean());     // alignment
    CHECK(bn254_pairing_check_batch_flags(nullptr, packed, k, mask, recs.data(), 0, nullptr, 99, F) == BN254_OK);
    CHECK(bn254_pairing_check_batch_flags(item.data(), packed, k, mask, recs.data(), 1, st.data(), 99, F) == BN254_E_BAD_ARG && clean());      // past the argument checks: the device ordinal
    CHECK(bn254_dbg_pairing_batch_rlc(item.data(), packed, k, mask, recs.data(), 1, nullptr, nullptr, nullptr, nullptr, st.data(), -1, 2) == BN254_E_BAD_ARG && clean());
    CHECK(g_pair_launches.load() == 0 && g_joint_launches.load() == 0);
  }
  // ---- host calls of three passes, packed and padded items, with and without shared positions: the records staged in front of every pass's items, one joint launch
  // per pass, the exact check behind the synchronisation for the groups the scatter fails; the counters
  for (auto shape : {std::pair<size_t, unsigned>{4, 0xEu}, std::pair<size_t, unsigned>{8, 0xAAu}, std::pair<size_t, unsigned>{2, 0x3u}, std::pair<size_t, unsigned>{3, 0x0u}}) {
    const size_t k = shape.first; const unsigned mask = shape.second;
    const size_t packed = bn254::pb_item_len((int)k, mask);
    const std::vector<uint8_t> recs = make_records(k, mask);
    for (size_t stride : {packed, packed + 9}) {
      const size_t pass = pb_host_pass_of(packed, recs.size(), 100000);
      CHECK(pass >= 64 && pass <= 1000);
      const size_t n = 2 * pass + 37;               // three passes, the last one below the knob's floor of 64
      std::vector<uint8_t> want, buf = marker_items(n, stride, pass, want), st(n + 1, 0xEE);
      const size_t jbefore = g_joint_launches.load();
      CHECK(bn254_pairing_rlc_state(s0) == 0);
      CHECK(bn254_pairing_check_batch_flags(buf.data(), stride, k, mask, mask ? recs.data() : nullptr, n, st.data(), 0, BN254_FLAG_RLC) == 0 && st[n] == 0xEE);
      CHECK(bn254_pairing_rlc_state(s1) == 0);
      CHECK(g_joint_launches.load() - jbefore == 2 && g_largest_launch.load() <= pass);
      const size_t groups = (pass + 63) / 64, failing = (groups + 12) / 16;
      CHECK(s1[0] - s0[0] == 2 && s1[1] - s0[1] == 2 * groups && s1[2] - s0[2] == 2 * failing && s1[3] - s0[3] == 1);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
      // flags == 0: the shared entry, no counter of this one moves
      CHECK(bn254_pairing_check_batch_flags(buf.data(), stride, k, mask, mask ? recs.data() : nullptr, n, st.data(), 0, 0) == 0 && bn254_pairing_rlc_state(s0) == 0);
      for (int q = 0; q < 4; q++) CHECK(s0[q] == s1[q]);
    }
  }
  // ---- the knob above n: the exact launches, out[3] alone; the device entry at and above a reservation, and with a corrupted record
  {
    const size_t k = 4; const unsigned mask = 0xE; const size_t stride = 400;
    std::vector<uint8_t> recs = make_records(k, mask);
    CHECK(bn254_pairing_reserve(100, 1) == 0);
    hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    bn254_set_pairing_rlc_params(251);
    for (size_t n : {(size_t)1, (size_t)100, (size_t)250}) {
      std::vector<uint8_t> want, buf = marker_items(n, stride, 1 << 18, want), st(n + 1, 0xEE);
      CHECK(bn254_pairing_rlc_state(s0) == 0);
      const size_t jbefore = g_joint_launches.load();
      CHECK(bn254_pairing_check_batch_flags_device(buf.data(), stride, k, mask, recs.data(), n, st.data(), 1, s, BN254_FLAG_RLC) == 0 && st[n] == 0xEE);
      CHECK(bn254_pairing_rlc_state(s1) == 0 && s1[0] == s0[0] && s1[1] == s0[1] && s1[2] == s0[2] && s1[3] - s0[3] == 1 && g_joint_launches.load() == jbefore);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    bn254_set_pairing_rlc_params(64);
    for (size_t n : {(size_t)64, (size_t)100, (size_t)250}) {
      std::vector<uint8_t> want, buf = marker_items(n, stride, 1 << 18, want), st(n + 3, 0xEE);
      CHECK(bn254_pairing_rlc_state(s0) == 0);
      CHECK(bn254_pairing_check_batch_flags_device(buf.data(), stride, k, mask, recs.data(), n, st.data() + 1, 1, s, BN254_FLAG_RLC) == 0 && st[0] == 0xEE && st[n + 1] == 0xEE);      // an odd status address
      CHECK(bn254_pairing_rlc_state(s1) == 0 && s1[0] - s0[0] == 1 && s1[1] - s0[1] == (n + 63) / 64 && s1[3] == s0[3]);
      for (size_t i = 0; i < n; i++) CHECK(st[i + 1] == want[i]);
    }
    std::vector<uint8_t> bad = recs; bad[0] ^= 1;
    std::vector<uint8_t> want, buf = marker_items(70, stride, 1 << 18, want), st(71, 0xEE);
    CHECK(bn254_pairing_check_batch_flags_device(buf.data(), stride, k, mask, bad.data(), 70, st.data(), 1, s, BN254_FLAG_RLC) == 0 && st[70] == 0xEE);
    for (size_t i = 0; i < 70; i++) CHECK(st[i] == BN254_ERR_MALFORMED);
    hipStreamDestroy(s);
  }
  // ---- the BN_HD bodies for real: the probe's host compile on small batches of real items (the weight step, the Miller run over the variable positions, the group
  // sums, the group product, the group check), two groups, with weights of the caller's and with all 1; then the probe on a stand-in device (the staged weights)
  for (auto shape : {std::pair<size_t, unsigned>{2, 0x3u}, std::pair<size_t, unsigned>{2, 0x2u}, std::pair<size_t, unsigned>{3, 0x0u}, std::pair<size_t, unsigned>{4, 0xEu}}) {
    const size_t k = shape.first; const unsigned mask = shape.second, n = 67, groups = 2;
    const size_t packed = bn254::pb_item_len((int)k, mask);
    const std::vector<uint8_t> recs = make_records(k, mask);
    std::vector<uint8_t> want, buf = real_items(n, k, mask, want), st(n + 1, 0xEE), igt(384 * n + 1, 0xEE), ggt(384 * groups + 1, 0xEE), gst(groups + 1, 0xEE), w(16 * n);
    for (size_t i = 0; i < w.size(); i++) w[i] = (uint8_t)(i * 37 + 11);
    for (const uint8_t* weights : {(const uint8_t*)w.data(), (const uint8_t*)nullptr}) {
      CHECK(bn254_dbg_pairing_batch_rlc(buf.data(), packed, k, mask, mask ? recs.data() : nullptr, n, weights, igt.data(), ggt.data(), gst.data(), st.data(), -1, 0) == 0);
      CHECK(st[n] == 0xEE && igt[384 * n] == 0xEE && ggt[384 * groups] == 0xEE && gst[groups] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
      CHECK(gst[0] == BN254_REJECT && gst[1] == BN254_REJECT);      // every group holds an item whose sign was dropped
    }
    CHECK(bn254_dbg_pairing_batch_rlc(buf.data(), packed, k, mask, mask ? recs.data() : nullptr, n, w.data(), igt.data(), ggt.data(), gst.data(), st.data(), 3, 0) == 0);
    CHECK(st[n] == 0xEE && igt[384 * n] == 0xEE && ggt[384 * groups] == 0xEE && gst[groups] == 0xEE);
  }
  // ---- an allocation failure at every allocation of a call, each on a device of its own that has passed its self-test: an error code, nothing written, and the same
  // call repeated without the failure answers right (nothing stale, nothing freed twice; leak detection is on)
  {
    const size_t n = 200, k = 4; const unsigned mask = 0xE; const size_t stride = bn254::pb_item_len((int)k, mask);
    std::vector<uint8_t> want, buf = marker_items(n, stride, 1 << 18, want), recs = make_records(k, mask);
    bool through = false;
    int dev = 4;
    for (size_t fail = 1; fail < 40 && !through; fail++, dev++) {
      unsigned m = 0; float ms = 0;
      CHECK(bn254_device_selftest(dev, &m, &ms) == 0);
      std::vector<uint8_t> st(n + 1, 0xEE);
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      const int rc = bn254_pairing_check_batch_flags(buf.data(), stride, k, mask, recs.data(), n, st.data(), dev, BN254_FLAG_RLC);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) through = true;
      else { CHECK(rc == BN254_E_HIP || rc == BN254_E_NOMEM); for (auto b : st) CHECK(b == 0xEE); }
      CHECK(bn254_pairing_check_batch_flags(buf.data(), stride, k, mask, recs.data(), n, st.data(), dev, BN254_FLAG_RLC) == 0 && st[n] == 0xEE);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want[i]);
    }
    CHECK(through && dev > 10);
  }
  // ---- two host threads on one device, one through the host entry and one through the device entry, with different masks, the knob moving beside them
  {
    const int dev = 46;
    std::atomic<int> bad{0};
    auto worker = [&](int which) {
      const size_t k = which ? 2 : 8; const unsigned mask = which ? 0x3u : 0xAAu;
      const std::vector<uint8_t> recs = make_records(k, mask);
      const size_t stride = bn254::pb_item_len((int)k, mask) + 4;
      for (int it = 0; it < 12; it++) {
        const size_t n = 30 + 37 * (size_t)it + (size_t)which;
        bn254_set_pairing_rlc_params(it % 3 ? 64 : 200);
        std::vector<uint8_t> want, buf = marker_items(n, stride, 1 << 18, want), st(n, 0xEE);
        const int rc = which ? bn254_pairing_check_batch_flags_device(buf.data(), stride, k, mask, recs.data(), n, st.data(), dev, nullptr, BN254_FLAG_RLC)
                             : bn254_pairing_check_batch_flags(buf.data(), stride, k, mask, recs.data(), n, st.data(), dev, BN254_FLAG_RLC);
        if (rc != 0 || st != want) bad++;
      }
    };
    std::thread t0(worker, 0), t1(worker, 1);
    t0.join(); t1.join();
    CHECK(bad.load() == 0);
  }
  printf("hostsan_pairing_rlc: %zu stand-in launches of the pairing batch, %zu joint launches, the largest of %zu items, %zu allocations still live (the per-device workspaces)\nhostsan_pairing_rlc ok\n",
         g_pair_launches.load(), g_joint_launches.load(), g_largest_launch.load(), g_fake_live_allocs.load());
  return 0;
}
