// Batches over many keys (csrc/bn254_capi_keys.hip) under the sanitizers: the host half of the library as ONE translation unit with the stand-in HIP runtime of
// hostsan_main.cpp (whose main is set aside), plus stand-ins for the launchers of the key-set pipeline.  The grouping is the real one (bn254_keys.h compiled for the
// host); the pipeline's stand-in reads every byte the kernels read -- record, input row of the key's width, descriptor -- so that a wrong size or a stale
// descriptor is an AddressSanitizer report, and answers REJECT for a record that starts with 0xEE, ACCEPT otherwise.
//   hostsan_keys <iterations> [threads]     (threads: only the concurrent scenarios, for the -fsanitize=thread build)
#include "hip/hip_runtime.h"
#include <cstddef>
static inline hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) { *free_b = (size_t)64 << 30; *total_b = (size_t)64 << 30; return hipSuccess; }
#define BN254_HOSTSAN_KEYS 1
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include <thread>

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
  g_launches++;
  for (size_t s = 0; s < a.m; s++) {
    a.slot_status[s] = 0;
    if (a.slot0 + s >= a.n_slots[0]) continue;
    const uint32_t pi = a.slot_to_proof[s];
    if (pi >= a.n_proofs) continue;
    const bn254::G16KeyDesc& d = a.desc[a.granule_key[s / G16_KEYS_GRANULE]];
    unsigned sum = 0;
    for (size_t b = 0; b < 256; b++) sum += a.proofs[(size_t)pi * a.stride + b];
    for (int b = 0; b < 32 * d.n_public; b++) sum += a.inputs[(size_t)pi * a.input_stride + b];
    sum += (unsigned)d.gtab[0] + (unsigned)d.dtab[BN_ATE_STEPS * FIXED_LINE_DWORDS - 1] + (unsigned)d.k0[17] + (unsigned)d.target[107];
    (void)a.ws[(s + 1) * (size_t)(G16_WS_BYTES_PER_PROOF / 4) - 1];
    a.status[pi] = a.proofs[(size_t)pi * a.stride] == 0xEE ? BN254_REJECT : (sum == 0xffffffffu ? BN254_REJECT : BN254_ACCEPT);
  }
  return hipSuccess;
}

static void make_key(uint64_t seed, size_t n_public, bn254_g16_pvk** out) {
  std::vector<uint8_t> vk(bn254_synth_groth16_vk_len(n_public)), p(256), in(32 * n_public + 1), e(1);
  CHECK(bn254_synth_groth16(seed, n_public, 1, 0, 1, 1, vk.data(), p.data(), in.data(), e.data()) == 0);
  CHECK(bn254_groth16_vk_prepare(vk.data(), vk.size(), 0, out) == 0);
}
// one mixed batch over `keys` (proof i under key i % n_keys, every 7th record marked invalid) through the host entry, checked
static void run_batch(const std::vector<bn254_g16_pvk*>& keys, size_t n, size_t input_stride, int device) {
  std::vector<uint8_t> proofs(256 * n, 1), rows(input_stride * n + 1, 2), st(n + 8, 0xAB);
  std::vector<unsigned> idx(n);
  for (size_t i = 0; i < n; i++) { idx[i] = (unsigned)(i * 7 % keys.size()); if (i % 7 == 3) proofs[256 * i] = 0xEE; }
  CHECK(bn254_groth16_verify_batch_keys(keys.data(), keys.size(), idx.data(), proofs.data(), 256, rows.data(), input_stride, n, st.data(), device, 0) == 0);
  for (size_t i = 0; i < n; i++) CHECK(st[i] == (i % 7 == 3 ? BN254_REJECT : BN254_ACCEPT));
  for (size_t i = n; i < n + 8; i++) CHECK(st[i] == 0xAB);
}

// An allocation failure at every allocation of bn254_groth16_reserve_keys and of a batch through the host and the device entry, raw and compressed records, on fresh
// keys (so: a fresh set) each time: an error code, the list still works afterwards, and -- leak detection, the count at exit -- the set owns whatever the call left
static void keys_alloc_failures() {
  const size_t n = 3000, widths[3] = {0, 2, 5};
  std::vector<uint8_t> vk(bn254_synth_groth16_vk_len(2)), raw(256 * 8), in8(64 * 8), ex(8), cp(128 * n), proofs(256 * n, 1), rows(512 * n + 1, 2), st(n + 8);
  CHECK(bn254_synth_groth16(0x5D0000, 2, 8, 0, 1, 1, vk.data(), raw.data(), in8.data(), ex.data()) == 0);
  for (size_t i = 0; i < n; i++) {     // gnark's compressed records of the eight proofs, repeated; every 7th does not decompress (compression flag 00 on A)
    uint8_t* r = &cp[128 * i];
    CHECK(bn254_g1_compress(&raw[256 * (i % 8)], r) == 0 && bn254_g2_compress(&raw[256 * (i % 8) + 64], r + 32) == 0 && bn254_g1_compress(&raw[256 * (i % 8) + 192], r + 96) == 0);
    if (i % 7 == 3) { r[0] &= 0x3f; proofs[256 * i] = 0xEE; }
  }
  std::vector<unsigned> idx(n);
  for (size_t i = 0; i < n; i++) idx[i] = (unsigned)(i * 7 % 3);
  for (int variant = 0; variant < 5; variant++) {
    const bool dev = variant & 1, cmp = variant & 2, reserve = variant == 4;
    bool through = false;
    for (size_t fail = 1; fail < 400 && !through; fail++) {
      std::vector<bn254_g16_pvk*> list(3);
      for (size_t k = 0; k < 3; k++) make_key(0x5E0000 + k, widths[k], &list[k]);
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      memset(st.data(), 0xAB, st.size());
      const uint8_t* p = cmp ? cp.data() : proofs.data(); const size_t stride = cmp ? 128 : 256; const unsigned flags = cmp ? BN254_FLAG_COMPRESSED_PROOFS : 0;
      const int rc = reserve ? bn254_groth16_reserve_keys(list.data(), 3, n, 0)
                     : dev   ? bn254_groth16_verify_batch_keys_device(list.data(), 3, idx.data(), p, stride, rows.data(), 512, n, st.data(), 0, nullptr, flags)
                             : bn254_groth16_verify_batch_keys(list.data(), 3, idx.data(), p, stride, rows.data(), 512, n, st.data(), 0, flags);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) {
        through = true;
        if (!reserve) for (size_t i = 0; i < n; i++) CHECK(st[i] == (i % 7 == 3 ? (cmp ? BN254_ERR_MALFORMED : BN254_REJECT) : BN254_ACCEPT));
      } else CHECK(rc == BN254_E_HIP || rc == BN254_E_NOMEM);
      CHECK(st[n] == 0xAB);
      run_batch(list, 300, 512, 0);     // the same list (the cached set the failed call left) still works
      for (auto k : list) bn254_groth16_vk_free(k);
    }
    CHECK(through);     // ended by a call that made every allocation, not by running out of iterations
  }
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 10;
  const bool threads_only = argc > 2 && std::string(argv[2]) == "threads";
  g_fake_device_count = 2;
  std::vector<bn254_g16_pvk*> keys(6);
  const size_t widths[6] = {0, 1, 2, 5, 16, 2};
  for (size_t k = 0; k < keys.size(); k++) make_key(0x5A0000 + k, widths[k], &keys[k]);
  if (!threads_only) {
    // sizes around the granule and the sub-batch cut; a list that names a handle twice; the set cache's eviction (more lists than slots) and re-use
    for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000, (size_t)70001}) run_batch(keys, n, 512, 0);
    for (long it = 0; it < iters; it++) {
      std::vector<bn254_g16_pvk*> list;
      for (size_t k = 0; k <= (size_t)it % 6; k++) list.push_back(keys[(it + k) % 6]);
      list.push_back(list[0]);
      CHECK(bn254_groth16_reserve_keys(list.data(), list.size(), 100 + 50 * it, it & 1) == 0);
      run_batch(list, 90 + 50 * it, 512, it & 1);
    }
    // freeing a member drops every cached list that contains it; preparing a new key (perhaps at the same address) and a new list is safe
    for (long it = 0; it < iters; it++) {
      bn254_g16_pvk* extra = nullptr;
      make_key(0x5B0000 + it, 2, &extra);
      std::vector<bn254_g16_pvk*> list = {keys[1], extra, keys[4]};
      run_batch(list, 300, 512, 0);
      bn254_groth16_vk_free(extra);
    }
    // refused lists and batches leave nothing behind
    std::vector<uint8_t> st(4, 0xAB); unsigned bad_idx[4] = {0, 9, 0, 0}; std::vector<uint8_t> pr(1024, 1), rows(2048, 0);
    CHECK(bn254_groth16_verify_batch_keys(keys.data(), keys.size(), bad_idx, pr.data(), 256, rows.data(), 512, 4, st.data(), 0, 0) == BN254_E_BAD_ARG && st[1] == 0xAB);
    CHECK(bn254_groth16_verify_batch_keys(keys.data(), keys.size(), bad_idx, pr.data(), 256, rows.data(), 511, 4, st.data(), 0, 0) == BN254_E_BAD_ARG);
    keys_alloc_failures();
  }
  // concurrent callers: the same list from several threads (serialised by the set's lock), different lists side by side (the cache's lock, eviction while a call
  // still holds an evicted set), and a thread that frees and re-prepares a member of its own lists meanwhile
  {
    std::vector<std::thread> th;
    for (int t = 0; t < 6; t++)
      th.emplace_back([&, t] {
        for (long it = 0; it < iters; it++) {
          if (t < 2) { run_batch(keys, 500 + 10 * t, 512, 0); continue; }
          if (t < 5) { std::vector<bn254_g16_pvk*> list = {keys[t % 6], keys[(t + it) % 6], keys[(t + 2 * it + 1) % 6]}; run_batch(list, 200 + t, 512, (int)(it & 1)); continue; }
          bn254_g16_pvk* own = nullptr;
          make_key(0x5C0000 + it, 1, &own);
          std::vector<bn254_g16_pvk*> list = {own, keys[2]};
          run_batch(list, 150, 64, 1);
          bn254_groth16_vk_free(own);
        }
      });
    for (auto& x : th) x.join();
  }
  for (auto k : keys) bn254_groth16_vk_free(k);
  printf("hostsan_keys: %ld stand-in launches, %zu allocations still live\nhostsan_keys ok\n", g_launches.load(), g_fake_live_allocs.load());
  return 0;
}
