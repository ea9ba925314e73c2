// The device self-test's host half (csrc/bn254_capi_selftest.hip: the gate, the per-device state, the entries, the comparison) under the sanitizers: the host half of
// the library as ONE translation unit with the stand-in HIP runtime and launchers of hostsan_main.cpp (whose main is set aside), plus a stand-in for the DEVICE half of
// the self-test (bn254_selftest_device) that this harness steers: it counts its runs per device, allocates and frees "device" memory as the real one does (so that an
// allocation can fail in the middle of a run), lets the host do its share (the key, the expected values), and hands back the expected bytes -- with one byte of check 4
// wrong on a device that is told to fail, and one byte of check k wrong when check k's input is not the pristine one (a fault injection of bn254_dbg_selftest).
//   hostsan_selftest [golden dir] [threads]     (threads: only the concurrent scenario, for the -fsanitize=thread build)
#include "hip/hip_runtime.h"
#define BN254_HOSTSAN_SELFTEST 1
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main
#include <thread>

static std::atomic<int> g_runs[16];
static std::atomic<int> g_fail_device{-1};      // the device whose check 4 disagrees (-1: none)
int bn254_selftest_device(int device, const std::vector<uint8_t> in[bn254st::CK_COUNT], const bn254st::HostSide& host, std::vector<uint8_t> got[bn254st::CK_COUNT],
                          float gpu_ms[bn254st::MS_COUNT]) {
  using namespace bn254st;
  int rc;
  CHECK(device >= 0 && device < 16 && t_fake_current_device == device);      // the caller made the device current
  g_runs[device]++;
  Stream stream; Event ev;
  PinBuf<uint8_t> h_in;
  DevBuf<uint8_t> d_in, d_out;
  DevBuf<int32_t> d_ws, d_key;
  size_t total = 0;
  for (int k = 0; k < CK_COUNT; k++) { CHECK(in[k].size() == in_bytes(k)); total += in[k].size(); }
  if ((rc = stream.ensure()) || (rc = ev.ensure_timed()) || (rc = h_in.ensure(total)) || (rc = d_in.ensure(total)) || (rc = d_out.ensure(4096)) || (rc = d_ws.ensure(256 * 1170)))
    return rc;
  size_t at = 0;
  for (int k = 0; k < CK_COUNT; k++) { memcpy(h_in + at, in[k].data(), in[k].size()); at += in[k].size(); }      // every input byte is read
  HIPCK(hipMemcpyAsync(d_in, h_in, total, hipMemcpyHostToDevice, stream));
  const Key* key = host.key();
  if (!key) return BN254_E_VK;
  CHECK(key->gtab.size() == (size_t)BN_ATE_STEPS * FIXED_LINE_DWORDS && key->dtab.size() == key->gtab.size() && key->kpts.size() == 36 && key->one.size() == 108);
  if ((rc = d_key.ensure(key->gtab.size() * 2 + 36 + 108 + 108 + 18))) return rc;      // the allocation in the middle of a run
  host.overlap();
  HIPCK(hipStreamSynchronize(stream));
  for (int k = 0; k < CK_COUNT; k++) {
    got[k] = bn254_selftest_expected(k);
    std::vector<uint8_t> pristine(in_bytes(k)), e(out_bytes(k));
    size_t a = 0, b = 0;
    CHECK(bn254_dbg_selftest_vectors(k, pristine.data(), pristine.size(), &a, e.data(), e.size(), &b) == 0 && a == pristine.size() && b == e.size() && e == got[k]);
    if (pristine != in[k]) got[k][0] ^= 1;
  }
  if (device == g_fail_device) got[CK_G16_LANE][0] ^= 1;
  for (int k = 0; k < MS_COUNT; k++) gpu_ms[k] = 0.f;
  return BN254_OK;
}

static void state_is(int device, int want_state, unsigned want_mask) {
  int st = 99; unsigned m = 99;
  CHECK(bn254_device_selftest_state(device, &st, &m) == 0);
  CHECK(st == want_state && m == want_mask);
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  const std::string golden = argc > 1 ? argv[1] : "tests/golden";
  const bool threads_only = argc > 2 && std::string(argv[2]) == "threads";
  g_fake_device_count = 8;
  g_fail_device = 3;
  const size_t n_public = 2, n = 64, pstride = 904;
  std::vector<uint8_t> vk(bn254_synth_groth16_vk_len(n_public)), proofs(256 * n), inputs(32 * n_public * n), expected(n);
  CHECK(bn254_synth_groth16(0xB2540000, n_public, n, 8, 1, 2, vk.data(), proofs.data(), inputs.data(), expected.data()) == 0);
  for (size_t i = 0; i < n; i += 5) proofs[256 * i] = 0xEE;                      // the stand-in's "invalid" mark: REJECT
  auto want = [&](size_t i) { return proofs[256 * i] == 0xEE ? BN254_REJECT : BN254_ACCEPT; };
  bn254_g16_pvk* pvk = nullptr;
  CHECK(bn254_groth16_vk_prepare(vk.data(), vk.size(), 0, &pvk) == 0);
  std::vector<uint8_t> pvkb = read_file(golden + "/plonk_vk.bin");
  CHECK(pvkb.size() == 34368);
  bn254_plonk_pvk* pk = nullptr;
  CHECK(bn254_plonk_vk_prepare(pvkb.data(), pvkb.size(), &pk) == 0);
  std::vector<uint8_t> pp(pstride * n, 1), pi(64 * n, 2);
  for (int d = 0; d < 8; d++) state_is(d, -1, 0);
  CHECK(g_fake_live_allocs == 0);

  // ---- six host threads make the first calls on all eight devices at once: one run per device, device 3 refuses, the others verify
  {
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    for (int t = 0; t < 6; t++)
      th.emplace_back([&, t] {
        for (int k = 0; k < 8; k++) {
          const int d = (k + t) % 8;
          std::vector<uint8_t> st(n + 8, 0xEE);
          const int rc = t % 2 == 0 ? bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), d, 0)
                                    : bn254_plonk_verify_batch(pk, pp.data(), pstride, pi.data(), 2, n, st.data(), d);
          if (d == 3) {
            if (rc != BN254_E_SELFTEST || !strstr(bn254_last_error(), "g16_lane")) bad++;
            for (size_t i = 0; i < n + 8; i++) if (st[i] != 0xEE) bad++;
          } else {
            if (rc != BN254_OK) bad++;
            for (size_t i = 0; i < n; i++) if (st[i] != (t % 2 == 0 ? want(i) : BN254_ACCEPT)) bad++;
            if (st[n] != 0xEE) bad++;
          }
        }
      });
    for (auto& x : th) x.join();
    CHECK(bad == 0);
    for (int d = 0; d < 8; d++) { CHECK(g_runs[d] == 1); state_is(d, d == 3 ? 0 : 1, d == 3 ? 1u << 4 : 0u); }
  }
  if (!threads_only) {
    // ---- every Groth16 and PlonK entry on the failed device: BN254_E_SELFTEST with the recorded text, no status byte, no run, nothing allocated there
    const size_t live = g_fake_live_allocs;
    std::vector<uint8_t> st(n + 8, 0xEE);
    auto refused = [&](int rc) {
      CHECK(rc == BN254_E_SELFTEST && strstr(bn254_last_error(), "check 4 (g16_lane)") && strstr(bn254_last_error(), "device 3"));
      for (size_t i = 0; i < n + 8; i++) CHECK(st[i] == 0xEE);
    };
    refused(bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 3, 0));
    refused(bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 3, BN254_FLAG_RLC));
    refused(bn254_groth16_verify_batch_device(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 3, nullptr, 0));
    refused(bn254_groth16_reserve(pvk, 4096, 3));
    refused(bn254_plonk_verify_batch(pk, pp.data(), pstride, pi.data(), 2, n, st.data(), 3));
    refused(bn254_plonk_verify_batch_flags(pk, pp.data(), pstride, pi.data(), 2, n, st.data(), 3, BN254_FLAG_RLC));
    refused(bn254_plonk_verify_batch_device(pk, pp.data(), pstride, pi.data(), 2, n, st.data(), 3, nullptr, 0));
    refused(bn254_plonk_reserve(pk, 4096, pstride, 3));
    // the multi-device entries report the device that refused; the other shards are complete
    {
      std::vector<uint8_t> ms(n + 8, 0xEE);
      CHECK(bn254_groth16_verify_batch_multi(pvk, proofs.data(), 256, inputs.data(), n_public, n, ms.data(), 0xFF, 0) != BN254_OK && strstr(bn254_last_error(), "g16_lane"));
      for (size_t i = 0; i < n; i++) CHECK(i / 8 == 3 ? ms[i] == 0xEE : ms[i] == want(i));
    }
    CHECK(g_runs[3] == 1 && g_fake_live_allocs == live);
    // an explicit run while the device still disagrees: the failure stays; a fault injection elsewhere does not touch a recorded state
    unsigned mask = 0; float t_ms = -1.f;
    CHECK(bn254_device_selftest(3, &mask, &t_ms) == BN254_E_SELFTEST && mask == 1u << 4 && t_ms >= 0.f && g_runs[3] == 2);
    state_is(3, 0, 1u << 4);
    CHECK(bn254_dbg_selftest(0, 7, 0, &mask) == BN254_E_SELFTEST && mask == 1u << 7 && strstr(bn254_last_error(), "pair2_coop"));
    state_is(0, 1, 0);
    CHECK(bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 0, 0) == BN254_OK);
    memset(st.data(), 0xEE, st.size());
    // recorded as the automatic run's would be: device 1 now refuses too, and a passing explicit run clears it
    CHECK(bn254_dbg_selftest(1, 9, 1, &mask) == BN254_E_SELFTEST && mask == 1u << 9);
    state_is(1, 0, 1u << 9);
    CHECK(bn254_plonk_verify_batch(pk, pp.data(), pstride, pi.data(), 2, n, st.data(), 1) == BN254_E_SELFTEST && strstr(bn254_last_error(), "sha256") && st[0] == 0xEE);
    CHECK(bn254_device_selftest(1, nullptr, nullptr) == BN254_OK);
    state_is(1, 1, 0);
    // the device computes correctly again: the explicit run passes, clears the failure, and the same batches verify
    g_fail_device = -1;
    refused(bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 3, 0));      // sticky until the explicit run
    CHECK(bn254_device_selftest(3, &mask, nullptr) == BN254_OK && mask == 0);
    state_is(3, 1, 0);
    CHECK(bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 3, 0) == BN254_OK);
    for (size_t i = 0; i < n; i++) CHECK(st[i] == want(i));
    CHECK(bn254_plonk_verify_batch(pk, pp.data(), pstride, pi.data(), 2, n, st.data(), 3) == BN254_OK);
    for (size_t i = 0; i < n; i++) CHECK(st[i] == BN254_ACCEPT);
    // ---- an allocation that fails at every point of an explicit run: the error is the runtime's, the state is untouched, nothing stays allocated
    {
      const size_t base = g_fake_live_allocs;
      int failures = 0;
      for (size_t k = 1;; k++) {
        g_fake_alloc_counter = 0; g_fake_fail_alloc_after = k;
        const int rc = bn254_device_selftest(5, &mask, nullptr);
        g_fake_fail_alloc_after = 0;
        CHECK(g_fake_live_allocs == base);
        state_is(5, 1, 0);
        if (rc == BN254_OK) break;
        CHECK(rc == BN254_E_HIP && mask == 0 && strstr(bn254_last_error(), "out of memory"));
        failures++;
        CHECK(k < 64);
      }
      CHECK(failures == 5);      // the five allocations of the stand-in above
    }
    // ... and of the AUTOMATIC run on a device not used yet: the first call fails with the runtime's error, records nothing, and the next call runs again and passes
    {
      g_fake_device_count = 9;
      const size_t base = g_fake_live_allocs;
      g_fake_alloc_counter = 0; g_fake_fail_alloc_after = 5;
      memset(st.data(), 0xEE, st.size());
      CHECK(bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 8, 0) == BN254_E_HIP && st[0] == 0xEE);
      g_fake_fail_alloc_after = 0;
      CHECK(g_fake_live_allocs == base && g_runs[8] == 1);
      state_is(8, -1, 0);
      CHECK(bn254_groth16_verify_batch(pvk, proofs.data(), 256, inputs.data(), n_public, n, st.data(), 8, 0) == BN254_OK && g_runs[8] == 2);
      state_is(8, 1, 0);
      for (size_t i = 0; i < n; i++) CHECK(st[i] == want(i));
    }
    // arguments
    int s0 = 0;
    CHECK(bn254_device_selftest(9, nullptr, nullptr) == BN254_E_BAD_ARG && bn254_device_selftest(-1, nullptr, nullptr) == BN254_E_BAD_ARG);
    CHECK(bn254_device_selftest_state(64, &s0, nullptr) == BN254_E_BAD_ARG && bn254_device_selftest_state(0, nullptr, nullptr) == BN254_E_BAD_ARG);
    CHECK(bn254_dbg_selftest(0, 10, 0, nullptr) == BN254_E_BAD_ARG && bn254_dbg_selftest(0, -2, 0, nullptr) == BN254_E_BAD_ARG);
    g_fake_device_count = 0;
    CHECK(bn254_device_selftest(0, nullptr, nullptr) == BN254_E_NO_DEVICE);
    g_fake_device_count = 9;
  }
  bn254_groth16_vk_free(pvk);
  bn254_plonk_vk_free(pk);
  CHECK(g_fake_live_allocs == 0);
  printf("hostsan_selftest ok\n");
  return 0;
}
