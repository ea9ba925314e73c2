// The synthetic PlonK workload generator (bn254_synth_plonk, _range, _for_inputs: csrc/bn254_capi_dbg.hip) under the sanitizers: the host half of the library as ONE
// translation unit with the stand-in HIP runtime of hostsan_main.cpp (whose main is set aside).  Every buffer is a heap allocation of exactly the documented size, so
// AddressSanitizer sees a write past a key, a record, an input row or a status byte; every proof then goes through the host compile of the verifier's first stage
// (bn254_plonk.hpp::plonk_stage1), which must answer what the generator expects up to the pairing check.  The generator touches no device: no stand-in launch is made.
//   hostsan_synth_plonk
#include "hip/hip_runtime.h"
#define main hostsan_base_main
#include "hostsan_main.cpp"
#undef main

struct Shape { size_t n_public, n_qcp; unsigned log2_size; };

// n proofs of a shape at a stride, every second one corrupted; returns how many the first stage lets through
static size_t run_shape(const Shape& s, size_t n, size_t stride, int threads) {
  const size_t plen = bn254_synth_plonk_proof_len(s.n_qcp), vlen = bn254_synth_plonk_vk_len(s.n_qcp);
  CHECK(plen == 808 + 96 * s.n_qcp && vlen == 34328 + 40 * s.n_qcp && stride >= plen);
  std::vector<uint8_t> vk(vlen), proofs(n * stride), inputs(n * s.n_public * 32), exp(n);
  CHECK(bn254_synth_plonk(0x5A0000 + s.log2_size, s.n_public, s.n_qcp, s.log2_size, n, 2, threads, vk.data(), n ? proofs.data() : nullptr, stride,
                          inputs.empty() ? nullptr : inputs.data(), n ? exp.data() : nullptr) == 0);
  PlonkKey key;
  CHECK(parse_plonk_vk(key, vk.data(), vk.size()) == DEC_OK && key.nb_public == s.n_public && key.n_qcp == s.n_qcp && key.size == (uint64_t)1 << s.log2_size);
  size_t through = 0;
  for (size_t i = 0; i < n; i++) {
    // an exact copy of the record and of the row: the stage reads nothing past either
    std::vector<uint8_t> rec(proofs.begin() + i * stride, proofs.begin() + i * stride + plen), row(inputs.begin() + i * s.n_public * 32, inputs.begin() + (i + 1) * s.n_public * 32);
    for (size_t k = plen; k < stride; k++) CHECK(proofs[i * stride + k] == 0);
    static const uint8_t none = 0;
    PlonkWork wk; std::vector<MsmTerm> terms(plonk_stage1_terms(key)); std::vector<uint8_t> fl(terms.size());
    wk.lambda = fr_ctx().one;
    const int st = plonk_stage1(key, rec.data(), rec.size(), row.empty() ? &none : row.data(), s.n_public, wk, terms.data(), fl.data());
    const int want = exp[i] == BN254_ACCEPT || exp[i] == BN254_ERR_PAIRING_FAILED ? (int)PL_OK : (int)exp[i];
    CHECK(st == want);
    if (st == PL_OK) through++;
  }
  // a range of the same stream is its slice
  if (n >= 8) {
    std::vector<uint8_t> vk2(vlen), p2(3 * stride), in2(3 * s.n_public * 32), e2(3);
    CHECK(bn254_synth_plonk_range(0x5A0000 + s.log2_size, s.n_public, s.n_qcp, s.log2_size, 5, 3, 2, 1, vk2.data(), p2.data(), stride, in2.empty() ? nullptr : in2.data(), e2.data()) == 0);
    CHECK(vk2 == vk && memcmp(p2.data(), proofs.data() + 5 * stride, 3 * stride) == 0 && memcmp(e2.data(), exp.data() + 5, 3) == 0);
    CHECK(in2.empty() || memcmp(in2.data(), inputs.data() + 5 * s.n_public * 32, in2.size()) == 0);
  }
  return through;
}

int main() {
  const long launches = g_launches.load();
  const Shape shapes[5] = {{0, 0, 3}, {1, 0, 10}, {2, 1, 26}, {3, 2, 20}, {5, 8, 28}};
  size_t through = 0, total = 0;
  for (const Shape& s : shapes) { through += run_shape(s, 24, bn254_synth_plonk_proof_len(s.n_qcp), 3); total += 24; }
  through += run_shape(shapes[4], 13, 1664, 4); total += 13;                    // a stride larger than the proof, more threads than a round of proofs divides into
  through += run_shape({0, 8, 3}, 12, 1576, 1); total += 12;                    // a domain of exactly n_public + n_qcp rows
  CHECK(run_shape(shapes[2], 0, 904, 2) == 0);                                  // n = 0: the key alone, no proof buffer
  CHECK(through > total / 2 && through < total);
  // proofs for rows the caller chose
  {
    std::vector<uint8_t> vk(bn254_synth_plonk_vk_len(1)), vk0(vk.size()), proofs(5 * 1000), rows(5 * 64, 0);
    for (size_t i = 0; i < rows.size(); i += 32) rows[i + 31] = (uint8_t)(i / 32);
    CHECK(bn254_synth_plonk_for_inputs(9, 2, 1, 26, 5, rows.data(), 2, vk.data(), proofs.data(), 1000) == 0);
    CHECK(bn254_synth_plonk(9, 2, 1, 26, 0, 0, 1, vk0.data(), nullptr, 904, nullptr, nullptr) == 0 && vk0 == vk);
    PlonkKey key;
    CHECK(parse_plonk_vk(key, vk.data(), vk.size()) == DEC_OK);
    for (size_t i = 0; i < 5; i++) {
      PlonkWork wk; std::vector<MsmTerm> terms(plonk_stage1_terms(key)); std::vector<uint8_t> fl(terms.size());
      wk.lambda = fr_ctx().one;
      std::vector<uint8_t> rec(proofs.begin() + i * 1000, proofs.begin() + i * 1000 + 904);
      CHECK(plonk_stage1(key, rec.data(), rec.size(), rows.data() + 64 * i, 2, wk, terms.data(), fl.data()) == PL_OK);
      CHECK(plonk_stage1(key, rec.data(), rec.size(), rows.data() + 64 * ((i + 1) % 5), 2, wk, terms.data(), fl.data()) == PL_OPENING);
    }
    std::vector<uint8_t> none_vk(bn254_synth_plonk_vk_len(0)), p0(2 * 808);
    CHECK(bn254_synth_plonk_for_inputs(9, 0, 0, 3, 2, nullptr, 1, none_vk.data(), p0.data(), 808) == 0);
  }
  // argument errors touch nothing: every buffer is one byte long
  {
    std::vector<uint8_t> vk(1, 0xC3), pr(1, 0xC3), in(1, 0xC3), ex(1, 0xC3);
    std::vector<uint8_t> big(64, 0xff);                                          // a row of values >= r
    const auto untouched = [&] { return vk[0] == 0xC3 && pr[0] == 0xC3 && in[0] == 0xC3 && ex[0] == 0xC3; };
    CHECK(bn254_synth_plonk(1, 2, 9, 26, 1, 2, 1, vk.data(), pr.data(), 4096, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, 2, 1, 0, 1, 2, 1, vk.data(), pr.data(), 904, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, 2, 1, 29, 1, 2, 1, vk.data(), pr.data(), 904, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, 6, 3, 3, 1, 2, 1, vk.data(), pr.data(), 4096, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, (size_t)-1, 1, 28, 1, 2, 1, vk.data(), pr.data(), 904, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, 2, 1, 26, 1, 2, 1, vk.data(), pr.data(), 903, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, 2, 1, 26, 1, 2, 1, nullptr, pr.data(), 904, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, 2, 1, 26, 1, 2, 1, vk.data(), nullptr, 904, in.data(), ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk(1, 2, 1, 26, 1, 2, 1, vk.data(), pr.data(), 904, nullptr, ex.data()) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk_range(1, 2, 1, 26, 3, 1, 2, 1, vk.data(), pr.data(), 904, in.data(), nullptr) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk_for_inputs(1, 2, 1, 26, 1, nullptr, 1, vk.data(), pr.data(), 904) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk_for_inputs(1, 2, 1, 26, 1, big.data(), 1, vk.data(), pr.data(), 904) == BN254_E_BAD_ARG);
    CHECK(bn254_synth_plonk_for_inputs(1, 2, 9, 26, 1, big.data(), 1, vk.data(), pr.data(), 4096) == BN254_E_BAD_ARG);
    CHECK(untouched());
  }
  CHECK(g_launches.load() == launches);
  printf("hostsan_synth_plonk: %zu of %zu proofs pass the first stage\nhostsan_synth_plonk ok\n", through, total);
  return 0;
}
