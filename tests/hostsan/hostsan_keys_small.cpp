// Small batches over many keys -- the direct form of csrc/bn254_capi_keys.hip (bn254_g16_plan.h::g16_keys_form) -- under the sanitizers: the host half of the library as
// ONE translation unit with the stand-in HIP runtime of hostsan_main.cpp (whose main is set aside), as hostsan_keys.cpp, plus stand-ins for ALL THREE launchers of
// the key-set path.  The host build starts with the knob at 0; this harness turns it to 30 720, so batches up to that size take the direct launcher.  Its stand-in
// reads every byte the kernels read -- the record, key_index[p], the input row of that key's width, one dword at each end of every table the descriptor points
// to, the last workspace dword of proof n - 1 -- so that a wrong size or a stale descriptor is an AddressSanitizer report; it answers MALFORMED for an index outside
// the list, REJECT for a record that starts with 0xEE, ACCEPT otherwise.
//   hostsan_keys_small <iterations> [threads]     (threads: only the concurrent scenario, for the -fsanitize=thread build)
#include "hip/hip_runtime.h"
#include <cstddef>
static inline hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) { *free_b = (size_t)64 << 30; *total_b = (size_t)64 << 30; return hipSuccess; }
#define BN254_HOSTSAN_KEYS 1
#define BN254_HOSTSAN_KEYS_DIRECT 1
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include <thread>

static std::atomic<long> g_direct{0}, g_grouped{0};

static unsigned read_desc(const bn254::G16KeyDesc& d) {
  unsigned sum = (unsigned)d.gtab[0] + (unsigned)d.gtab[BN_ATE_STEPS * FIXED_LINE_DWORDS - 1] + (unsigned)d.dtab[0] + (unsigned)d.dtab[BN_ATE_STEPS * FIXED_LINE_DWORDS - 1] +
                 (unsigned)d.k0[0] + (unsigned)d.k0[17] + (unsigned)d.target[0] + (unsigned)d.target[107];
  if (d.n_public > 0) sum += (unsigned)d.msm_tab[0] + (unsigned)d.msm_tab[(size_t)d.n_public * 32 * 255 * MSM_ENTRY_DWORDS - 1];
  return sum;
}
hipError_t bn254_launch_keys_group(const uint32_t* key_index, uint32_t n, uint32_t n_keys, uint32_t slot_cap, uint32_t* count, uint32_t* base, uint32_t* cursor, uint32_t* n_slots,
                                   uint32_t* slot_to_proof, uint32_t* granule_key, uint8_t* status, hipStream_t) {
  g_launches++;
  for (uint32_t s = 0; s < slot_cap; s++) slot_to_proof[s] = G16_KEYS_NO_PROOF;
  for (uint32_t g = 0; g < slot_cap / G16_KEYS_GRANULE + 1; g++) granule_key[g] = 0;
  for (uint32_t i = 0; i < n; i++) if (key_index[i] >= n_keys) status[i] = BN254_ERR_MALFORMED;
  n_slots[0] = bn254::keys_group_host(key_index, n, n_keys, slot_to_proof, granule_key, count, base);
  for (uint32_t k = 0; k < n_keys; k++) cursor[k] = base[k];
  return hipSuccess;
}
hipError_t bn254_launch_g16_keys(const G16KeysLaunchArgs& a, hipStream_t) {
  g_launches++; g_grouped++;
  for (size_t s = 0; s < a.m; s++) {
    a.slot_status[s] = 0;
    if (a.slot0 + s >= a.n_slots[0]) continue;
    const uint32_t pi = a.slot_to_proof[s];
    if (pi >= a.n_proofs) continue;
    const bn254::G16KeyDesc& d = a.desc[a.granule_key[s / G16_KEYS_GRANULE]];
    unsigned sum = read_desc(d);
    for (size_t b = 0; b < 256; b++) sum += a.proofs[(size_t)pi * a.stride + b];
    for (int b = 0; b < 32 * d.n_public; b++) sum += a.inputs[(size_t)pi * a.input_stride + b];
    (void)a.ws[(s + 1) * (size_t)(G16_WS_BYTES_PER_PROOF / 4) - 1];
    a.status[pi] = a.proofs[(size_t)pi * a.stride] == 0xEE ? BN254_REJECT : (sum == 0xffffffffu ? BN254_REJECT : BN254_ACCEPT);
  }
  return hipSuccess;
}
hipError_t bn254_launch_g16_keys_direct(const G16KeysDirectArgs& a, hipStream_t) {
  g_launches++; g_direct++;
  if (a.n == 0 || a.n > (size_t)COOP12_MAX_PROOFS) return hipErrorInvalidDevice;      // the plan never sends such a batch here
  (void)a.ws[a.n * (size_t)(G16_WS_BYTES_PER_PROOF / 4) - 1];
  for (size_t p = 0; p < a.n; p++) {
    const uint32_t k = a.key_index[p];
    unsigned sum = 0;
    for (size_t b = 0; b < 256; b++) sum += a.proofs[p * a.stride + b];
    if (k >= a.n_keys) { a.status[p] = BN254_ERR_MALFORMED; continue; }
    const bn254::G16KeyDesc& d = a.desc[k];
    sum += read_desc(d);
    for (int b = 0; b < 32 * d.n_public; b++) sum += a.inputs[p * a.input_stride + b];
    a.status[p] = a.proofs[p * a.stride] == 0xEE ? BN254_REJECT : (sum == 0xffffffffu ? BN254_REJECT : BN254_ACCEPT);
  }
  return hipSuccess;
}

static void make_key(uint64_t seed, size_t n_public, bn254_g16_pvk** out) {
  std::vector<uint8_t> vk(bn254_synth_groth16_vk_len(n_public)), p(256), in(32 * n_public + 1), e(1);
  CHECK(bn254_synth_groth16(seed, n_public, 1, 0, 1, 1, vk.data(), p.data(), in.data(), e.data()) == 0);
  CHECK(bn254_groth16_vk_prepare(vk.data(), vk.size(), 0, out) == 0);
}
static int last_form(const std::vector<bn254_g16_pvk*>& keys, int device) {
  int f = -2;
  CHECK(bn254_dbg_g16_keys_last_form(keys.data(), keys.size(), device, &f) == 0);
  return f;
}
// The compressed form of eight valid proofs, repeated; every 7th record does not decompress (compression flag 00 on A)
struct Records {
  std::vector<uint8_t> raw, cmp, rows;
  explicit Records(size_t n) : raw(256 * n, 1), cmp(128 * n), rows(512 * n + 1, 2) {
    std::vector<uint8_t> vk(bn254_synth_groth16_vk_len(2)), r8(256 * 8), in8(64 * 8), ex(8);
    CHECK(bn254_synth_groth16(0x5F0000, 2, 8, 0, 1, 1, vk.data(), r8.data(), in8.data(), ex.data()) == 0);
    uint8_t c8[8][128];
    for (size_t j = 0; j < 8; j++) CHECK(bn254_g1_compress(&r8[256 * j], c8[j]) == 0 && bn254_g2_compress(&r8[256 * j + 64], c8[j] + 32) == 0 && bn254_g1_compress(&r8[256 * j + 192], c8[j] + 96) == 0);
    for (size_t i = 0; i < n; i++) {
      memcpy(&cmp[128 * i], c8[i % 8], 128);
      if (i % 7 == 3) { cmp[128 * i] &= 0x3f; raw[256 * i] = 0xEE; }
    }
  }
};
// one mixed batch (proof i under key i * 7 % n_keys, every 7th record invalid) through one entry; bad_index: position of an index outside the list (device entry), or n
static void run_batch(const std::vector<bn254_g16_pvk*>& keys, const Records& r, size_t n, bool dev, bool cmp, int device, int want_form, size_t bad_index = (size_t)-1) {
  std::vector<uint8_t> st(n + 8, 0xAB);
  std::vector<unsigned> idx(n);
  for (size_t i = 0; i < n; i++) idx[i] = (unsigned)(i * 7 % keys.size());
  if (bad_index < n) idx[bad_index] = (unsigned)keys.size() + 3;
  const uint8_t* p = cmp ? r.cmp.data() : r.raw.data(); const size_t stride = cmp ? 128 : 256; const unsigned flags = cmp ? BN254_FLAG_COMPRESSED_PROOFS : 0;
  const int rc = dev ? bn254_groth16_verify_batch_keys_device(keys.data(), keys.size(), idx.data(), p, stride, r.rows.data(), 512, n, st.data(), device, nullptr, flags)
                     : bn254_groth16_verify_batch_keys(keys.data(), keys.size(), idx.data(), p, stride, r.rows.data(), 512, n, st.data(), device, flags);
  if (bad_index < n && !dev) { CHECK(rc == BN254_E_BAD_ARG); for (size_t i = 0; i < n + 8; i++) CHECK(st[i] == 0xAB); return; }
  CHECK(rc == 0);
  for (size_t i = 0; i < n; i++) CHECK(st[i] == (i == bad_index || (cmp && i % 7 == 3) ? BN254_ERR_MALFORMED : i % 7 == 3 ? BN254_REJECT : BN254_ACCEPT));
  for (size_t i = n; i < n + 8; i++) CHECK(st[i] == 0xAB);
  if (want_form >= 0) CHECK(last_form(keys, device) == want_form);
}

// An allocation failure at every allocation of a direct-form batch through the host and the device entry, raw and compressed records, on fresh keys (so: a fresh
// set) each time: an error code, the list still works afterwards, and -- leak detection, the count at exit -- the set owns whatever the call left
static void alloc_failures(const Records& r) {
  const size_t n = 3000, widths[3] = {0, 2, 5};
  for (int variant = 0; variant < 4; variant++) {
    const bool dev = variant & 1, cmp = variant & 2;
    bool through = false;
    for (size_t fail = 1; fail < 400 && !through; fail++) {
      std::vector<bn254_g16_pvk*> list(3);
      for (size_t k = 0; k < 3; k++) make_key(0x5E1000 + k, widths[k], &list[k]);
      std::vector<uint8_t> st(n + 8, 0xAB);
      std::vector<unsigned> idx(n);
      for (size_t i = 0; i < n; i++) idx[i] = (unsigned)(i * 7 % 3);
      const uint8_t* p = cmp ? r.cmp.data() : r.raw.data(); const size_t stride = cmp ? 128 : 256; const unsigned flags = cmp ? BN254_FLAG_COMPRESSED_PROOFS : 0;
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      const int rc = dev ? bn254_groth16_verify_batch_keys_device(list.data(), 3, idx.data(), p, stride, r.rows.data(), 512, n, st.data(), 0, nullptr, flags)
                         : bn254_groth16_verify_batch_keys(list.data(), 3, idx.data(), p, stride, r.rows.data(), 512, n, st.data(), 0, flags);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) {
        through = true;
        for (size_t i = 0; i < n; i++) CHECK(st[i] == (i % 7 == 3 ? (cmp ? BN254_ERR_MALFORMED : BN254_REJECT) : BN254_ACCEPT));
        CHECK(last_form(list, 0) == 1);
      } else CHECK(rc == BN254_E_HIP || rc == BN254_E_NOMEM);
      CHECK(st[n] == 0xAB);
      run_batch(list, r, 300, false, false, 0, 1);     // the same list (the cached set the failed call left) still works
      for (auto k : list) bn254_groth16_vk_free(k);
    }
    CHECK(through);     // ended by a call that made every allocation, not by running out of iterations
  }
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 10;
  const bool threads_only = argc > 2 && std::string(argv[2]) == "threads";
  g_fake_device_count = 2;
  int form = -1; size_t slots = 0; int launches = 0;
  CHECK(bn254_dbg_g16_keys_plan(300, 6, &form, &slots, &launches) == 0 && form == 0);      // a host build starts with the grouped form at every size
  bn254_set_keys_params(30720);
  CHECK(bn254_dbg_g16_keys_plan(300, 6, &form, &slots, &launches) == 0 && form == 1 && slots == 300 && launches == 2);
  std::vector<bn254_g16_pvk*> keys(6);
  const size_t widths[6] = {0, 1, 2, 5, 16, 2};
  for (size_t k = 0; k < keys.size(); k++) make_key(0x5A1000 + k, widths[k], &keys[k]);
  const Records r(30721);
  if (!threads_only) {
    CHECK(last_form(keys, 0) == -1);
    // the boundaries of a wavefront and of the direct form, both entries, raw and compressed records
    for (size_t n : {(size_t)1, (size_t)5, (size_t)6, (size_t)300, (size_t)30720, (size_t)30721})
      for (int v = 0; v < 4; v++) run_batch(keys, r, n, v & 1, v & 2, 0, n <= 30720 ? 1 : 0);
    CHECK(g_direct.load() == 20 && g_grouped.load() >= 4);
    // an index outside the list: the device entry answers MALFORMED for that proof (first, inside, last), the host entry refuses the vector
    for (size_t bad : {(size_t)0, (size_t)3, (size_t)299}) { run_batch(keys, r, 300, true, false, 0, 1, bad); run_batch(keys, r, 300, false, false, 0, -1, bad); }
    // a reservation smaller than a later batch, then one larger than it; a list that names a handle twice; more lists than cache slots
    for (long it = 0; it < iters; it++) {
      std::vector<bn254_g16_pvk*> list;
      for (size_t k = 0; k <= (size_t)it % 6; k++) list.push_back(keys[(it + k) % 6]);
      list.push_back(list[0]);
      CHECK(bn254_groth16_reserve_keys(list.data(), list.size(), 40 + 10 * it, it & 1) == 0);
      run_batch(list, r, 300 + 50 * it, it & 2, it & 4, it & 1, 1);
      CHECK(bn254_groth16_reserve_keys(list.data(), list.size(), 1000, it & 1) == 0);
      const size_t live = g_fake_live_allocs.load();
      run_batch(list, r, 1000, true, false, it & 1, 1);
      CHECK(g_fake_live_allocs.load() == live);          // after the reservation a device call allocates nothing
    }
    // the knob flipped between batches on one cached list: the workspace of the reservation serves both forms
    CHECK(bn254_groth16_reserve_keys(keys.data(), keys.size(), 2000, 0) == 0);
    {
      const size_t live = g_fake_live_allocs.load();
      for (long it = 0; it < iters; it++) {
        const bool direct = !(it & 1);
        bn254_set_keys_params(direct ? 30720 : 0);
        run_batch(keys, r, 2000 - (size_t)it, true, false, 0, direct ? 1 : 0);
        bn254_set_keys_params(direct ? 1999 - it : 2000 - it);            // the hand-over exactly at the batch's size
        run_batch(keys, r, 2000 - (size_t)it, true, false, 0, direct ? 0 : 1);
      }
      CHECK(g_fake_live_allocs.load() == live);
      bn254_set_keys_params(-1);                                          // leaves the knob alone
      bn254_set_keys_params(1000000);                                     // clamped
      CHECK(bn254_dbg_g16_keys_plan(30720, 6, &form, &slots, &launches) == 0 && form == 1);
      CHECK(bn254_dbg_g16_keys_plan(30721, 6, &form, &slots, &launches) == 0 && form == 0);
    }
    alloc_failures(r);
  }
  // concurrent callers with the knob on (the six-thread scenario of hostsan_keys.cpp): the same list from several threads, different lists side by side on both
  // fake devices (eviction while a call still holds an evicted set), a thread that frees and re-prepares a member of its own lists, and one that moves the knob
  {
    std::vector<std::thread> th;
    for (int t = 0; t < 6; t++)
      th.emplace_back([&, t] {
        for (long it = 0; it < iters; it++) {
          if (t < 2) { run_batch(keys, r, 500 + 10 * t, t & 1, false, 0, -1); continue; }
          if (t < 5) {
            std::vector<bn254_g16_pvk*> list = {keys[t % 6], keys[(t + it) % 6], keys[(t + 2 * it + 1) % 6]};
            run_batch(list, r, 200 + t, it & 2, it & 4, (int)(it & 1), -1);
            if (t == 4) bn254_set_keys_params(it & 1 ? 30720 : 203);
            continue;
          }
          bn254_g16_pvk* own = nullptr;
          make_key(0x5C1000 + it, 1, &own);
          std::vector<bn254_g16_pvk*> list = {own, keys[2]};
          run_batch(list, r, 150, false, false, 1, -1);
          bn254_groth16_vk_free(own);
        }
      });
    for (auto& x : th) x.join();
  }
  for (auto k : keys) bn254_groth16_vk_free(k);
  printf("hostsan_keys_small: %ld stand-in launches (%ld direct, %ld grouped), %zu allocations still live\nhostsan_keys_small ok\n", g_launches.load(), g_direct.load(), g_grouped.load(),
         g_fake_live_allocs.load());
  return 0;
}
