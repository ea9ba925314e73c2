// BN254_FLAG_RLC over PlonK key lists (csrc/bn254_capi_plonk_keys.hip::pk_run_pass) under the sanitizers: the host half of the library as ONE translation unit
// with the stand-in HIP runtime of hostsan_main.cpp (whose main is set aside), the stand-ins of hostsan_plonk_keys.cpp for the launchers of a pass -- stage 2 counts
// the launches that come with a weight key -- and a stand-in for the launcher the flag adds: the joint check of a pass's groups, which reads the descriptor's line
// tables of EVERY group's key, the target and the whole group workspace, and writes every group's status byte.  The group stage of hostsan_main.cpp makes group g of a pass fail when g % 16 == 3, so a
// pass of 16 granules and more runs the exact check behind the joint one and a smaller pass does not.  The threshold is set to 64 slots here; the older harness
// stays below the default and never reaches these launchers.
//   hostsan_plonk_keys_rlc <iterations> [threads]     (threads: only the concurrent scenario, for the -fsanitize=thread build)
#include "hip/hip_runtime.h"
#include <cstddef>
static inline hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) { *free_b = (size_t)64 << 30; *total_b = (size_t)64 << 30; return hipSuccess; }
#define BN254_HOSTSAN_PLONK_KEYS 1
#define BN254_HOSTSAN_PLONK_KEYS_RLC 1
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include "../../snark-bn254-verifier_amd/csrc/bn254_capi_plonk_keys.hip"
#include <thread>

static std::atomic<long> g_weighted{0}, g_group_checks{0}, g_exact{0};
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
static const bn254::PlonkKeyDesc& desc_of(const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, size_t slot) {
  const uint32_t k = granule_key[slot / G16_KEYS_GRANULE];
  return desc[k < n_keys ? k : 0];
}
hipError_t bn254_launch_plonk_keys_gather(const uint8_t* proofs, size_t stride, const uint8_t* inputs, size_t input_stride, uint32_t n_proofs, const uint32_t* slot_to_proof,
                                          const uint32_t* granule_key, const bn254::PlonkKeyDesc* desc, uint32_t n_keys, uint32_t m, uint8_t* recs, uint32_t rec_stride, uint32_t rec_bytes,
                                          uint8_t* rows, uint32_t row_stride, hipStream_t) {
  g_launches++;
  for (uint32_t j = 0; j < m; j++) {
    const uint32_t pi = slot_to_proof[j];
    memset(recs + (size_t)j * rec_stride, 0, rec_stride);
    if (row_stride) memset(rows + (size_t)j * row_stride, 0, row_stride);
    if (pi >= n_proofs) continue;
    memcpy(recs + (size_t)j * rec_stride, proofs + (size_t)pi * stride, rec_bytes);
    const size_t in_bytes = 32 * (size_t)desc_of(desc, n_keys, granule_key, j).n_public;
    CHECK(in_bytes <= row_stride);
    if (in_bytes) memcpy(rows + (size_t)j * row_stride, inputs + (size_t)pi * input_stride, in_bytes);      // nothing behind the key's inputs is read
  }
  return hipSuccess;
}
hipError_t bn254_launch_plonk_stage1_keys(const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const uint8_t* d_recs, size_t rec_stride, size_t proof_len,
                                          const uint8_t* d_inputs, size_t in_stride, size_t staged_public, size_t n, const uint32_t* lam_key, void* d_work, void* d_terms, uint8_t* d_flags,
                                          int T1, hipStream_t) {
  g_launches++;
  lam_record(lam_key);
  CHECK(n % 64 == 0 && proof_len >= 808 && staged_public <= 8);
  unsigned sum = 0;
  for (size_t i = 0; i < n; i++) {
    const bn254::PlonkKeyDesc& d = desc_of(desc, n_keys, granule_key, i);
    sum += ((const uint8_t*)d.key)[sizeof(PlonkKey) - 1];
    for (size_t b = 0; b < rec_stride; b++) sum += d_recs[i * rec_stride + b];
    for (size_t b = 0; b < 32 * (size_t)d.n_public; b++) sum += d_inputs[i * in_stride + b];
  }
  memset(d_work, (int)(sum & 1), n * sizeof(PlonkWork)); memset(d_terms, 0, n * (size_t)T1 * sizeof(MsmTerm)); memset(d_flags, 0, n * (size_t)T1);
  return hipSuccess;
}
hipError_t bn254_launch_plonk_stage2_keys(const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const uint8_t* d_recs, size_t rec_stride, size_t n, void*,
                                          const uint32_t* words, const uint8_t* inf, void* d_terms, uint8_t* d_flags, uint8_t* d_status, int TT, int, const uint32_t* weight_key,
                                          hipStream_t) {
  g_launches++;
  if (weight_key) { g_weighted++; (void)weight_key[10]; }
  (void)words[n * 16 - 1]; (void)inf[n - 1];
  memset(d_terms, 0, n * (size_t)TT * sizeof(MsmTerm)); memset(d_flags, 0, n * (size_t)TT);
  for (size_t i = 0; i < n; i++) {
    (void)((const uint8_t*)desc_of(desc, n_keys, granule_key, i).key)[0];
    const uint8_t* r = d_recs + i * rec_stride;
    bool zero = true;
    for (size_t b = 0; b < rec_stride && zero; b++) zero = r[b] == 0;
    d_status[i] = zero ? (uint8_t)BN254_ERR_MALFORMED : r[0] == 0xEE ? (uint8_t)BN254_ERR_OPENING_MISMATCH : (uint8_t)BN254_ST_PENDING;
  }
  return hipSuccess;
}
hipError_t bn254_launch_g1_msm_rows_keys(const MsmPlan& plan, const int32_t* terms, const uint8_t* flags, size_t n, int n_terms, int32_t* part, int32_t* glv_tab,
                                         const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, hipStream_t) {
  g_launches++;
  (void)terms[n * (size_t)n_terms * MSM_TERM_DWORDS - 1]; (void)flags[n * (size_t)n_terms - 1];
  for (size_t i = 0; i < n; i += 64) (void)desc_of(desc, n_keys, granule_key, i).fixed_tabs[0];
  memset(part, 0x11, (size_t)plan.n_rows * 27 * n * sizeof(int32_t));
  memset(glv_tab, 0x12, bn254_g1_msm_scratch_lanes(plan, n) * (size_t)G1_GLV_TAB_BYTES_PER_LANE);
  return hipSuccess;
}
hipError_t bn254_launch_pairing2_fixed_keys(int32_t* ws, uint8_t* status, size_t n, const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const int32_t* one,
                                            int, hipStream_t) {
  g_launches++;
  (void)one[12 * BN_NL - 1]; (void)ws[n * (size_t)(G16_WS_BYTES_PER_PROOF / 4) - 1];
  for (size_t i = 0; i < n; i++) {
    const bn254::PlonkKeyDesc& d = desc_of(desc, n_keys, granule_key, i);
    (void)d.tab0[BN_ATE_STEPS * FIXED_LINE_DWORDS - 1]; (void)d.tab1[BN_ATE_STEPS * FIXED_LINE_DWORDS - 1];
    if (status[i] & BN254_ST_PENDING) status[i] = BN254_ST_ACCEPT;
  }
  return hipSuccess;
}
hipError_t bn254_launch_plonk_keys_scatter(const uint8_t* slot_status, const uint32_t* slot_to_proof, uint32_t m, uint32_t n_proofs, uint8_t* status, hipStream_t) {
  g_launches++;
  for (uint32_t j = 0; j < m; j++) if (slot_to_proof[j] < n_proofs) status[slot_to_proof[j]] = slot_status[j];
  return hipSuccess;
}

hipError_t bn254_launch_pairing2_fixed_groups_keys(int32_t* grp_ws, uint8_t* grp_status, size_t groups, const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key,
                                                   const int32_t* one, int reject_code, hipStream_t) {
  g_launches++; g_group_checks++;
  CHECK(groups >= 1 && groups <= COOP12_MAX_PROOFS_FIXED);
  (void)one[12 * BN_NL - 1];
  unsigned sum = 0;
  for (size_t w = 0; w < groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4); w++) sum += (unsigned)grp_ws[w];
  for (size_t g = 0; g < groups; g++) {
    const uint32_t k = granule_key[g];      // key_shift 0: one word per group
    const bn254::PlonkKeyDesc& d = desc[k < n_keys ? k : 0];
    sum += (unsigned)d.tab0[BN_ATE_STEPS * FIXED_LINE_DWORDS - 1] + (unsigned)d.tab1[BN_ATE_STEPS * FIXED_LINE_DWORDS - 1];
    if (grp_status[g] & BN254_ST_PENDING) grp_status[g] = (g % 16) == 3 ? (uint8_t)reject_code : (uint8_t)(BN254_ST_ACCEPT | (sum & 0));
  }
  return hipSuccess;
}

static void make_key(uint64_t seed, size_t n_public, size_t n_qcp, bn254_plonk_pvk** out) {
  std::vector<uint8_t> vk(bn254_synth_plonk_vk_len(n_qcp)), p(bn254_synth_plonk_proof_len(n_qcp)), in(32 * n_public + 1), e(1);
  CHECK(bn254_synth_plonk(seed, n_public, n_qcp, 6, 1, 0, 1, vk.data(), p.data(), p.size(), in.data(), e.data()) == 0);
  CHECK(bn254_plonk_vk_prepare(vk.data(), vk.size(), out) == 0);
}
#define PK_STRIDE 1000
static unsigned flags_of(bool rlc) { return rlc ? (unsigned)BN254_FLAG_RLC : 0u; }
// one mixed batch over `keys` (proof i under key 7 i % n_keys, every 7th record marked invalid) through the host or the device entry, checked: the status bytes are
// those of the exact path whatever the flag
static void run_batch(const std::vector<bn254_plonk_pvk*>& keys, size_t n, size_t input_stride, int device, bool dev_entry, bool rlc) {
  std::vector<uint8_t> proofs(PK_STRIDE * n, 1), rows(input_stride * n + 1, 2), st(n + 8, 0xAB);
  std::vector<unsigned> idx(n);
  for (size_t i = 0; i < n; i++) { idx[i] = (unsigned)(i * 7 % keys.size()); if (i % 7 == 3) proofs[PK_STRIDE * i] = 0xEE; }
  const int rc = dev_entry ? bn254_plonk_verify_batch_keys_device(keys.data(), keys.size(), idx.data(), proofs.data(), PK_STRIDE, rows.data(), input_stride, n, st.data(), device, nullptr, flags_of(rlc))
                           : bn254_plonk_verify_batch_keys(keys.data(), keys.size(), idx.data(), proofs.data(), PK_STRIDE, rows.data(), input_stride, n, st.data(), device, flags_of(rlc));
  CHECK(rc == 0);
  for (size_t i = 0; i < n; i++) CHECK(st[i] == (i % 7 == 3 ? BN254_ERR_OPENING_MISMATCH : BN254_ACCEPT));
  for (size_t i = n; i < n + 8; i++) CHECK(st[i] == 0xAB);
}
struct State { uint64_t v[4]; };
static State state_of(const std::vector<bn254_plonk_pvk*>& keys, int device) { State s; CHECK(bn254_plonk_keys_state(keys.data(), keys.size(), device, s.v) == 0); return s; }

// An allocation failure at every allocation of a batch with the flag through the host and the device entry, on fresh keys each time: an error code, the list still
// works afterwards with and without the flag, and -- leak detection -- the set owns whatever the call left
static void rlc_alloc_failures() {
  const size_t n = 1100, widths[3] = {0, 2, 5};
  std::vector<uint8_t> proofs(PK_STRIDE * n, 1), rows(160 * n + 1, 2), st(n + 8);
  std::vector<unsigned> idx(n);
  for (size_t i = 0; i < n; i++) { idx[i] = (unsigned)(i * 7 % 3); if (i % 7 == 3) proofs[PK_STRIDE * i] = 0xEE; }
  for (int variant = 0; variant < 2; variant++) {
    bool through = false;
    for (size_t fail = 1; fail < 600 && !through; fail++) {
      std::vector<bn254_plonk_pvk*> list(3);
      for (size_t k = 0; k < 3; k++) make_key(0x7E0000 + k, widths[k], 1, &list[k]);
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = fail;
      memset(st.data(), 0xAB, st.size());
      const int rc = variant ? bn254_plonk_verify_batch_keys_device(list.data(), 3, idx.data(), proofs.data(), PK_STRIDE, rows.data(), 160, n, st.data(), 0, nullptr, BN254_FLAG_RLC)
                             : bn254_plonk_verify_batch_keys(list.data(), 3, idx.data(), proofs.data(), PK_STRIDE, rows.data(), 160, n, st.data(), 0, BN254_FLAG_RLC);
      g_fake_fail_alloc_after = 0;
      if (rc == 0) {
        through = true;
        for (size_t i = 0; i < n; i++) CHECK(st[i] == (i % 7 == 3 ? BN254_ERR_OPENING_MISMATCH : BN254_ACCEPT));
      } else CHECK(rc == BN254_E_HIP || rc == BN254_E_NOMEM);
      CHECK(st[n] == 0xAB);
      run_batch(list, 200, 160, 0, false, true);     // the same list (the cached set the failed call left) still works
      run_batch(list, 200, 160, 0, true, false);
      for (auto k : list) bn254_plonk_vk_free(k);
    }
    CHECK(through);     // ended by a call that made every allocation, not by running out of iterations
  }
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 6;
  const bool threads_only = argc > 2 && std::string(argv[2]) == "threads";
  g_fake_device_count = 2;
  bn254_set_plonk_rlc_params(64);
  std::vector<bn254_plonk_pvk*> keys(5);
  const size_t widths[5] = {0, 1, 2, 5, 2};
  for (size_t k = 0; k < keys.size(); k++) make_key(0x7A0000 + k, widths[k], 1, &keys[k]);
  if (!threads_only) {
    uint64_t none[4];
    CHECK(bn254_plonk_keys_state(keys.data(), keys.size(), 0, none) == BN254_E_BAD_ARG);      // not cached yet
    CHECK(bn254_plonk_keys_state(nullptr, 5, 0, none) == BN254_E_BAD_ARG && bn254_plonk_keys_state(keys.data(), 5, 0, nullptr) == BN254_E_BAD_ARG);
    run_batch(keys, 1, 160, 0, false, false);
    // passes without a failed group (fewer than four granules... up to 15), with one (16 granules and more), two chains (above 5040 slots); both entries
    for (size_t n : {(size_t)1, (size_t)64, (size_t)65, (size_t)300, (size_t)700, (size_t)1100, (size_t)4800, (size_t)5100}) {
      for (int dev_entry = 0; dev_entry < 2; dev_entry++) {
        const State a = state_of(keys, 0);
        const long w0 = g_weighted.load(), gc0 = g_group_checks.load();
        run_batch(keys, n, 160, 0, dev_entry != 0, true);
        const State b = state_of(keys, 0);
        const uint64_t passes = b.v[0] - a.v[0], groups = b.v[1] - a.v[1], failed = b.v[2] - a.v[2];
        CHECK(passes >= 1 && passes == (uint64_t)(g_weighted.load() - w0) && passes == (uint64_t)(g_group_checks.load() - gc0));
        CHECK(groups >= (n + 63) / 64 && groups <= (n + 63 * 5) / 64 + 5);
        if (passes == 1) CHECK(failed == (groups + 12) / 16);      // groups 3, 19, .. of the one pass
        else CHECK(failed >= 1);
        // the flag without effect below the threshold: no counter moves
        bn254_set_plonk_rlc_params(1 << 20);
        run_batch(keys, n, 160, 0, dev_entry != 0, true);
        const State c = state_of(keys, 0);
        CHECK(c.v[0] == b.v[0] && c.v[1] == b.v[1] && c.v[2] == b.v[2]);
        bn254_set_plonk_rlc_params(64);
      }
    }
    // the setters clamp and leave alone
    long kn[2];
    bn254_set_plonk_rlc_params(1); CHECK(bn254_dbg_plonk_keys_knobs(kn) == 0 && kn[1] == 64);
    bn254_set_plonk_rlc_params(-1); CHECK(bn254_dbg_plonk_keys_knobs(kn) == 0 && kn[1] == 64);
    bn254_set_plonk_keys_params(1L << 40); CHECK(bn254_dbg_plonk_keys_knobs(kn) == 0 && kn[0] == COOP12_MAX_PROOFS_FIXED);
    bn254_set_plonk_keys_params(0); bn254_set_plonk_keys_params(-5); CHECK(bn254_dbg_plonk_keys_knobs(kn) == 0 && kn[0] == 0);
    bn254_set_plonk_keys_params(COOP12_MAX_PROOFS_FIXED);
    // a member freed: the cached list goes, its state with it
    {
      bn254_plonk_pvk* extra = nullptr;
      make_key(0x7B0000, 2, 1, &extra);
      std::vector<bn254_plonk_pvk*> list = {keys[1], extra, keys[3]};
      run_batch(list, 1100, 160, 1, false, true);
      CHECK(state_of(list, 1).v[0] == 1);
      bn254_plonk_vk_free(extra);
      uint64_t out[4];
      CHECK(bn254_plonk_keys_state(list.data(), list.size(), 1, out) == BN254_E_BAD_ARG);
    }
    rlc_alloc_failures();
  }
  // two host threads on one list, one with the flag and one without (contexts leased side by side, the counters shared), a third on two other lists, one per fake device
  {
    std::vector<std::thread> th;
    for (int t = 0; t < 3; t++)
      th.emplace_back([&, t] {
        for (long it = 0; it < iters; it++) {
          if (t < 2) { run_batch(keys, 1100 + 10 * t, 160, 0, t == 1, t == 0); continue; }
          std::vector<bn254_plonk_pvk*> list = {keys[2], keys[3 + (it & 1)]};      // two lists: with the shared one, fewer than the cache's four slots, so nothing is evicted
          run_batch(list, 1100, 160, (int)(it & 1), false, (it & 1) != 0);
        }
      });
    for (auto& x : th) x.join();
    CHECK(state_of(keys, 0).v[0] >= (uint64_t)iters);
  }
  for (auto k : keys) bn254_plonk_vk_free(k);
  CHECK(lam_all_fresh());
  printf("hostsan_plonk_keys_rlc: %ld stand-in launches, %ld joint checks, %zu allocations still live\nhostsan_plonk_keys_rlc ok\n", g_launches.load(), g_group_checks.load(), g_fake_live_allocs.load());
  return 0;
}
