// bn254_verify.hpp -- the host side of the drop-in, in C++: the crate's surface (verifier/src/lib.rs:27-74) over the C ABI of bn254_verify.h.
//
// The reference is a Rust crate; a Rust host binds the C ABI directly.  This header is the same surface for a C++ host and
// the place where the mapping "status byte -> what the reference does" is written down once:
//
//   reference (Rust)                                                        here (C++17, header only)
//   Groth16Verifier::verify(proof, vk, public_inputs) -> Result<bool, _>    snark_bn254_verifier::Groth16Verifier::verify(...) -> Result<bool, Groth16Error>
//   PlonkVerifier::verify(proof, vk, public_inputs) -> Result<bool, _>      snark_bn254_verifier::PlonkVerifier::verify(...)   -> Result<bool, PlonkError>
//   (new) verify_batch(&[proof], &vk, &[[Fr]])                              Groth16Verifier::verify_batch / PlonkVerifier::verify_batch -> status bytes
//   public_inputs: &[bn::Fr] built with Fr::from_slice(32 big-endian bytes) Fr = std::array<uint8_t, 32>, big-endian
//   .unwrap() of a loader error (lib.rs:45-46, 70-71): a panic              throws Panic (carries the status byte that names the loader error)
//   Ok(true) / Ok(false) / Err(e)                                           Result::ok() + value / error()
//
// Groth16 (groth16/verify.rs:53-78): ACCEPT = Ok(true), REJECT = Ok(false), ERR_INPUT_LEN = Err(PrepareInputsFailed); proof coordinates that
// are no field members / not on the curve / B outside G2 / short buffers are the loaders' errors, i.e. panics.
// PlonK (plonk/verify.rs:46-317, kzg.rs:180-187): ACCEPT = Ok(true); the verifier never answers Ok(false): a failed check is
// Err(OpeningPolyMismatch | PairingCheckFailed | Bsb22CommitmentMismatch | InverseNotFound | InvalidWitness).
//
// Everything runs on the GPU through libbn254_verify_amd.so; without a usable device the calls throw InfrastructureError (BN254_E_NO_DEVICE):
// there is no CPU path.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <memory>
#include <vector>
#include "bn254_verify.h"

namespace snark_bn254_verifier {

using Fr = std::array<uint8_t, 32>;   // what bn::Fr::from_slice reads: 32 big-endian bytes (any 256-bit value; used modulo r, examples/script/src/main.rs:204-213)
using Bytes = std::vector<uint8_t>;

// groth16/error.rs
enum class Groth16Error { ProofVerificationFailed, ProcessVerifyingKeyFailed, PrepareInputsFailed, UnexpectedIdentity, GeneralError };
// plonk/error.rs: the variants verify_plonk can return on well-formed buffers
enum class PlonkError { Bsb22CommitmentMismatch, InverseNotFound, InvalidWitness, OpeningPolyMismatch, PairingCheckFailed, GeneralError };

inline const char* to_string(Groth16Error e) {
  switch (e) {
    case Groth16Error::ProofVerificationFailed: return "Proof verification failed";
    case Groth16Error::ProcessVerifyingKeyFailed: return "Process verifying key failed";
    case Groth16Error::PrepareInputsFailed: return "Prepare inputs failed";
    case Groth16Error::UnexpectedIdentity: return "Unexpected identity";
    default: return "General error";
  }
}
inline const char* to_string(PlonkError e) {
  switch (e) {
    case PlonkError::Bsb22CommitmentMismatch: return "BSB22 Commitment number mismatch";
    case PlonkError::InverseNotFound: return "Inverse not found";
    case PlonkError::InvalidWitness: return "Invalid witness";
    case PlonkError::OpeningPolyMismatch: return "Opening linear polynomial mismatch";
    case PlonkError::PairingCheckFailed: return "Pairing check failed";
    default: return "General error";
  }
}

// where the reference unwrap()s a loader error: the status byte says which (BN254_ERR_NOT_MEMBER, _NOT_ON_CURVE, _NOT_IN_SUBGROUP, _MALFORMED)
struct Panic : std::runtime_error {
  int status;
  explicit Panic(int st) : std::runtime_error(std::string("called `Result::unwrap()` on an `Err` value: ") + bn254_status_string(st)), status(st) {}
};
// the library could not run (no device, HIP error, bad argument): not an outcome of the proof
struct InfrastructureError : std::runtime_error {
  int code;
  explicit InfrastructureError(int c) : std::runtime_error(std::string("bn254_verify: ") + bn254_last_error()), code(c) {}
};
// BN254_E_SELFTEST: a shipped kernel disagrees with its known answer on the device, which is refused until a device_selftest on it passes; what() names the check
struct SelfTestError : InfrastructureError {
  explicit SelfTestError() : InfrastructureError(BN254_E_SELFTEST) {}
};

template <class T, class E>
class Result {   // Result<bool, Groth16Error> / Result<bool, PlonkError>
 public:
  static Result Ok(T v) { Result r; r.ok_ = true; r.value_ = v; return r; }
  static Result Err(E e) { Result r; r.ok_ = false; r.err_ = e; return r; }
  bool ok() const { return ok_; }
  bool is_err() const { return !ok_; }
  T value() const { if (!ok_) throw std::logic_error("Result: value() on Err"); return value_; }
  E error() const { if (ok_) throw std::logic_error("Result: error() on Ok"); return err_; }
  T unwrap() const { if (!ok_) throw std::runtime_error(std::string("called `Result::unwrap()` on an `Err` value: ") + to_string(err_)); return value_; }

 private:
  bool ok_ = false;
  T value_{};
  E err_{};
};

namespace detail {
inline void check(int rc) { if (rc == BN254_E_SELFTEST) throw SelfTestError(); if (rc != BN254_OK) throw InfrastructureError(rc); }
inline Bytes flatten(const std::vector<Fr>& v) { Bytes b(32 * v.size()); for (size_t i = 0; i < v.size(); i++) std::copy(v[i].begin(), v[i].end(), b.begin() + 32 * i); return b; }
inline Result<bool, Groth16Error> groth16_outcome(int st) {
  switch (st) {
    case BN254_ACCEPT: return Result<bool, Groth16Error>::Ok(true);
    case BN254_REJECT: return Result<bool, Groth16Error>::Ok(false);
    case BN254_ERR_INPUT_LEN: return Result<bool, Groth16Error>::Err(Groth16Error::PrepareInputsFailed);
    default: throw Panic(st);
  }
}
inline Result<bool, PlonkError> plonk_outcome(int st) {
  switch (st) {
    case BN254_ACCEPT: return Result<bool, PlonkError>::Ok(true);
    case BN254_ERR_OPENING_MISMATCH: return Result<bool, PlonkError>::Err(PlonkError::OpeningPolyMismatch);
    case BN254_ERR_PAIRING_FAILED: return Result<bool, PlonkError>::Err(PlonkError::PairingCheckFailed);
    case BN254_ERR_BSB22_MISMATCH: return Result<bool, PlonkError>::Err(PlonkError::Bsb22CommitmentMismatch);
    case BN254_ERR_INVERSE: return Result<bool, PlonkError>::Err(PlonkError::InverseNotFound);
    case BN254_ERR_INPUT_LEN: return Result<bool, PlonkError>::Err(PlonkError::InvalidWitness);
    default: throw Panic(st);
  }
}
// proofs of different lengths side by side: records of the longest length (>= min_len), shorter ones zero-padded and remembered
inline Bytes pack(const std::vector<Bytes>& proofs, size_t min_len, size_t* stride, std::vector<bool>* is_short) {
  size_t s = min_len;
  for (const auto& p : proofs) s = p.size() > s ? p.size() : s;
  Bytes b(s * proofs.size(), 0);
  is_short->assign(proofs.size(), false);
  for (size_t i = 0; i < proofs.size(); i++) { std::copy(proofs[i].begin(), proofs[i].end(), b.begin() + s * i); (*is_short)[i] = proofs[i].size() < min_len; }
  *stride = s;
  return b;
}
}  // namespace detail

namespace detail {
// the host buffers of an SP1 batch: values concatenated, n + 1 offsets, vkey hashes (one for all: stride 0; one per proof: stride 32)
struct Sp1Buffers {
  Bytes pv, vk; std::vector<uint64_t> offs; size_t n, stride;
  Sp1Buffers(const std::vector<std::array<uint8_t, 32>>& vkey_hashes, const std::vector<Bytes>& public_values) : n(public_values.size()) {
    if (vkey_hashes.size() != 1 && vkey_hashes.size() != n) throw std::invalid_argument("one vkey hash, or one per proof");
    offs.reserve(n + 1);
    for (const Bytes& v : public_values) { offs.push_back(pv.size()); pv.insert(pv.end(), v.begin(), v.end()); }
    offs.push_back(pv.size());
    if (pv.empty()) pv.push_back(0);
    for (const auto& h : vkey_hashes) vk.insert(vk.end(), h.begin(), h.end());
    stride = (vkey_hashes.size() == 1 && n != 1) ? 0 : 32;
  }
};
}  // namespace detail
// SP1's committed_values_digest: SHA-256(public_values) with the top three bits of byte 0 cleared (the circuit's input 1; input 0 is the program's vkey hash)
inline std::array<uint8_t, 32> sp1_public_values_digest(const Bytes& public_values) {
  std::array<uint8_t, 32> out{};
  detail::check(bn254_sp1_public_values_digest(public_values.data(), public_values.size(), out.data()));
  return out;
}

// A verifying key prepared once (decompression, e(alpha, beta), line tables, window tables: the work lib.rs:46 and groth16/verify.rs:70 repeat per call)
class PreparedGroth16Vk {
 public:
  explicit PreparedGroth16Vk(const Bytes& vk, unsigned mode = BN254_VK_REFERENCE) {
    int rc = bn254_groth16_vk_prepare(vk.data(), vk.size(), mode, &h_);
    if (rc == BN254_E_VK) throw Panic(BN254_ERR_MALFORMED);            // load_groth16_verifying_key_from_bytes(vk).unwrap()
    detail::check(rc);
  }
  ~PreparedGroth16Vk() { if (h_) bn254_groth16_vk_free(h_); }
  PreparedGroth16Vk(const PreparedGroth16Vk&) = delete;
  PreparedGroth16Vk& operator=(const PreparedGroth16Vk&) = delete;
  PreparedGroth16Vk(PreparedGroth16Vk&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  size_t num_public() const { return bn254_groth16_vk_num_public(h_); }
  const bn254_g16_pvk* handle() const { return h_; }
  // n records of `stride` bytes, n_public x 32 bytes of inputs per proof; one status byte per proof (bn254_verify.h)
  Bytes verify_batch(const uint8_t* proofs, size_t stride, const uint8_t* public_inputs, size_t n_public, size_t n, int device = 0, unsigned flags = 0) const {
    Bytes st(n ? n : 1);
    detail::check(bn254_groth16_verify_batch(h_, proofs, stride, public_inputs, n_public, n, st.data(), device, flags));
    st.resize(n);
    return st;
  }
  // SP1 proofs from their public values: proof i verified against vkey_hashes[i] (or the one hash) | SHA-256(public_values[i]) & mask, the digest made on the device
  Bytes verify_sp1_batch(const uint8_t* proofs, size_t stride, const std::vector<std::array<uint8_t, 32>>& vkey_hashes, const std::vector<Bytes>& public_values,
                         int device = 0, unsigned flags = 0) const {
    detail::Sp1Buffers b(vkey_hashes, public_values);
    Bytes st(b.n ? b.n : 1);
    detail::check(bn254_sp1_groth16_verify_batch(h_, proofs, stride, b.vk.data(), b.stride, b.pv.data(), b.offs.data(), b.n, st.data(), device, flags));
    st.resize(b.n);
    return st;
  }
  Bytes verify_batch_multi(const uint8_t* proofs, size_t stride, const uint8_t* public_inputs, size_t n_public, size_t n, uint64_t device_mask, unsigned flags = 0) const {
    Bytes st(n ? n : 1);
    detail::check(bn254_groth16_verify_batch_multi(h_, proofs, stride, public_inputs, n_public, n, st.data(), device_mask, flags));
    st.resize(n);
    return st;
  }
  // enqueues on hip_stream and returns (BN254_FLAG_RLC: after one stream synchronisation)
  void verify_batch_device(const void* d_proofs, size_t stride, const void* d_public_inputs, size_t n_public, size_t n, void* d_status, int device = 0, void* hip_stream = nullptr,
                           unsigned flags = 0) const {
    detail::check(bn254_groth16_verify_batch_device(h_, d_proofs, stride, d_public_inputs, n_public, n, d_status, device, hip_stream, flags));
  }
  void reserve(size_t n, int device = 0) const { detail::check(bn254_groth16_reserve(h_, n, device)); }
  // takes over a handle the library made (Groth16Verifier::prepare_batch)
  static PreparedGroth16Vk adopt(bn254_g16_pvk* h) { PreparedGroth16Vk k; k.h_ = h; return k; }

 private:
  PreparedGroth16Vk() = default;
  bn254_g16_pvk* h_ = nullptr;
};

struct Groth16Verifier {
  // Many keys prepared in one call, on `device` (bn254_groth16_vk_prepare_batch): entry i is the prepared key vks[i], equal to PreparedGroth16Vk(vks[i], mode) in
  // everything a caller can observe, or empty for a key that does not load (where the single-key constructor throws Panic).  The keys are independent of each other.
  static std::vector<std::unique_ptr<PreparedGroth16Vk>> prepare_batch(const std::vector<Bytes>& vks, unsigned mode = BN254_VK_REFERENCE, int device = 0) {
    const size_t n = vks.size();
    std::vector<const uint8_t*> ptrs(n); std::vector<size_t> lens(n); std::vector<bn254_g16_pvk*> out(n, nullptr); std::vector<int> status(n, 0);
    static const uint8_t none = 0;
    for (size_t i = 0; i < n; i++) { ptrs[i] = vks[i].empty() ? &none : vks[i].data(); lens[i] = vks[i].size(); }
    detail::check(bn254_groth16_vk_prepare_batch(ptrs.data(), lens.data(), n, mode, device, out.data(), status.data()));
    std::vector<std::unique_ptr<PreparedGroth16Vk>> keys(n);
    for (size_t i = 0; i < n; i++) if (out[i]) keys[i].reset(new PreparedGroth16Vk(PreparedGroth16Vk::adopt(out[i])));
    return keys;
  }
  // lib.rs:44-49
  static Result<bool, Groth16Error> verify(const Bytes& proof, const Bytes& vk, const std::vector<Fr>& public_inputs, unsigned mode = BN254_VK_REFERENCE) {
    uint8_t st = 0xEE;
    const Bytes in = detail::flatten(public_inputs);
    int rc = bn254_groth16_verify(proof.data(), proof.size(), vk.data(), vk.size(), in.data(), public_inputs.size(), mode, &st);
    if (rc == BN254_E_VK) throw Panic(BN254_ERR_MALFORMED);
    detail::check(rc);
    return detail::groth16_outcome(st);
  }
  // the batch entry: one status byte per proof (BN254_ACCEPT, BN254_REJECT, BN254_ERR_*); outcome() turns a byte into the reference's answer
  static Bytes verify_batch(const std::vector<Bytes>& proofs, const Bytes& vk, const std::vector<std::vector<Fr>>& public_inputs,
                            unsigned mode = BN254_VK_REFERENCE, int device = 0, unsigned flags = 0) {
    if (proofs.size() != public_inputs.size()) throw std::invalid_argument("verify_batch: one input vector per proof");
    PreparedGroth16Vk pvk(vk, mode);
    const size_t n = proofs.size(), n_public = n ? public_inputs[0].size() : 0;
    Bytes in(32 * n_public * n);
    for (size_t i = 0; i < n; i++) {
      if (public_inputs[i].size() != n_public) throw std::invalid_argument("verify_batch: the proofs of a batch share the number of public inputs");
      const Bytes f = detail::flatten(public_inputs[i]);
      std::copy(f.begin(), f.end(), in.begin() + 32 * n_public * i);
    }
    size_t stride; std::vector<bool> is_short;
    const Bytes pb = detail::pack(proofs, 256, &stride, &is_short);
    Bytes st = pvk.verify_batch(pb.data(), stride, in.data(), n_public, n, device, flags);
    for (size_t i = 0; i < n; i++) if (is_short[i]) st[i] = BN254_ERR_MALFORMED;      // a buffer the loader cannot slice: a panic in the reference
    return st;
  }
  // one batch over many keys (bn254_verify.h, "Batches over many keys"): proof i is verified against keys[key_index[i]]; its inputs are the first
  // 32 x num_public(that key) bytes of row i of public_inputs (input_stride bytes per row).  Keys with more than 16 public inputs are refused.
  static Bytes verify_batch_keys(const std::vector<const PreparedGroth16Vk*>& keys, const std::vector<unsigned>& key_index, const uint8_t* proofs, size_t stride,
                                 const uint8_t* public_inputs, size_t input_stride, int device = 0, unsigned flags = 0) {
    std::vector<const bn254_g16_pvk*> h(keys.size());
    for (size_t k = 0; k < keys.size(); k++) h[k] = keys[k] ? keys[k]->handle() : nullptr;
    Bytes st(key_index.size());
    detail::check(bn254_groth16_verify_batch_keys(h.data(), h.size(), key_index.data(), proofs, stride, public_inputs, input_stride, key_index.size(), st.data(), device, flags));
    return st;
  }
  static void reserve_keys(const std::vector<const PreparedGroth16Vk*>& keys, size_t n, int device = 0) {
    std::vector<const bn254_g16_pvk*> h(keys.size());
    for (size_t k = 0; k < keys.size(); k++) h[k] = keys[k] ? keys[k]->handle() : nullptr;
    detail::check(bn254_groth16_reserve_keys(h.data(), h.size(), n, device));
  }
  // the plan of a batch over many keys (bn254_set_keys_params): batches of up to coop_max proofs take the direct cooperative form; 0: always the grouped form;
  // a negative value leaves the knob alone.  Process-wide.
  static void set_keys_params(long coop_max) { bn254_set_keys_params(coop_max); }
  static Result<bool, Groth16Error> outcome(uint8_t status) { return detail::groth16_outcome(status); }
};

class PreparedPlonkVk {
 public:
  explicit PreparedPlonkVk(const Bytes& vk) {
    int rc = bn254_plonk_vk_prepare(vk.data(), vk.size(), &h_);
    if (rc == BN254_E_VK) throw Panic(BN254_ERR_MALFORMED);            // load_plonk_verifying_key_from_bytes(vk).unwrap()
    detail::check(rc);
  }
  ~PreparedPlonkVk() { if (h_) bn254_plonk_vk_free(h_); }
  PreparedPlonkVk(const PreparedPlonkVk&) = delete;
  PreparedPlonkVk& operator=(const PreparedPlonkVk&) = delete;
  size_t num_public() const { return bn254_plonk_vk_num_public(h_); }
  // flags: BN254_FLAG_RLC batches the pairing checks of a pass across proofs (same status bytes; honoured from 8192 proofs per pass)
  Bytes verify_batch(const uint8_t* proofs, size_t stride, const uint8_t* public_inputs, size_t n_public, size_t n, int device = 0, unsigned flags = 0) const {
    Bytes st(n ? n : 1);
    detail::check(bn254_plonk_verify_batch_flags(h_, proofs, stride, public_inputs, n_public, n, st.data(), device, flags));
    st.resize(n);
    return st;
  }
  // SP1 proofs from their public values, as PreparedGroth16Vk::verify_sp1_batch (flags: BN254_FLAG_RLC only)
  Bytes verify_sp1_batch(const uint8_t* proofs, size_t stride, const std::vector<std::array<uint8_t, 32>>& vkey_hashes, const std::vector<Bytes>& public_values,
                         int device = 0, unsigned flags = 0) const {
    detail::Sp1Buffers b(vkey_hashes, public_values);
    Bytes st(b.n ? b.n : 1);
    detail::check(bn254_sp1_plonk_verify_batch(h_, proofs, stride, b.vk.data(), b.stride, b.pv.data(), b.offs.data(), b.n, st.data(), device, flags));
    st.resize(b.n);
    return st;
  }
  // the same over the GPUs selected by device_mask (contiguous shards, one host thread per device)
  Bytes verify_batch_multi(const uint8_t* proofs, size_t stride, const uint8_t* public_inputs, size_t n_public, size_t n, uint64_t device_mask, unsigned flags = 0) const {
    Bytes st(n ? n : 1);
    detail::check(bn254_plonk_verify_batch_multi(h_, proofs, stride, public_inputs, n_public, n, st.data(), device_mask, flags));
    st.resize(n);
    return st;
  }
  // proofs, inputs and status bytes in device memory; returns when the status bytes are in d_status (bn254_verify.h)
  void verify_batch_device(const void* d_proofs, size_t stride, const void* d_public_inputs, size_t n_public, size_t n, void* d_status, int device = 0, void* hip_stream = nullptr,
                           unsigned flags = 0) const {
    detail::check(bn254_plonk_verify_batch_device(h_, d_proofs, stride, d_public_inputs, n_public, n, d_status, device, hip_stream, flags));
  }
  void reserve(size_t n, size_t proof_stride = 0, int device = 0) const { detail::check(bn254_plonk_reserve(h_, n, proof_stride, device)); }
  const bn254_plonk_pvk* handle() const { return h_; }

 private:
  bn254_plonk_pvk* h_ = nullptr;
};

struct PlonkVerifier {
  // lib.rs:69-74
  static Result<bool, PlonkError> verify(const Bytes& proof, const Bytes& vk, const std::vector<Fr>& public_inputs) {
    uint8_t st = 0xEE;
    const Bytes in = detail::flatten(public_inputs);
    int rc = bn254_plonk_verify(proof.data(), proof.size(), vk.data(), vk.size(), in.data(), public_inputs.size(), &st);
    if (rc == BN254_E_VK) throw Panic(BN254_ERR_MALFORMED);
    detail::check(rc);
    return detail::plonk_outcome(st);
  }
  static Bytes verify_batch(const std::vector<Bytes>& proofs, const Bytes& vk, const std::vector<std::vector<Fr>>& public_inputs, int device = 0) {
    if (proofs.size() != public_inputs.size()) throw std::invalid_argument("verify_batch: one input vector per proof");
    PreparedPlonkVk pvk(vk);
    const size_t n = proofs.size(), n_public = n ? public_inputs[0].size() : 0;
    Bytes in(32 * n_public * n);
    for (size_t i = 0; i < n; i++) {
      if (public_inputs[i].size() != n_public) throw std::invalid_argument("verify_batch: the proofs of a batch share the number of public inputs");
      const Bytes f = detail::flatten(public_inputs[i]);
      std::copy(f.begin(), f.end(), in.begin() + 32 * n_public * i);
    }
    size_t stride; std::vector<bool> is_short;
    const Bytes pb = detail::pack(proofs, 516, &stride, &is_short);
    Bytes st = pvk.verify_batch(pb.data(), stride, in.data(), n_public, n, device);
    // a proof shorter than its own layout (plonk/converter.rs:121-178: 8 points, count + claimed values, second opening, count + commitments) is a slice-index panic in
    // the reference; padded to the stride it would parse as something else
    for (size_t i = 0; i < n; i++) {
      const Bytes& p = proofs[i];
      auto be32 = [&p](size_t o) { return (size_t)p[o] << 24 | (size_t)p[o + 1] << 16 | (size_t)p[o + 2] << 8 | (size_t)p[o + 3]; };
      bool bad = p.size() < 516;
      if (!bad) { const size_t off = 516 + 32 * be32(512); bad = p.size() < off + 100 || p.size() < off + 100 + 64 * be32(off + 96); }
      if (bad) st[i] = BN254_ERR_MALFORMED;
    }
    return st;
  }
  // one batch over many keys (bn254_verify.h, "PlonK batches over many keys"): proof i is verified against keys[key_index[i]]; its inputs are the first
  // 32 * num_public(that key) bytes of row i of public_inputs (rows input_stride bytes apart).  At most 256 keys, all with the same number of BSB22 commitments
  static Bytes verify_batch_keys(const std::vector<const PreparedPlonkVk*>& keys, const std::vector<unsigned>& key_index, const uint8_t* proofs, size_t stride,
                                 const uint8_t* public_inputs, size_t input_stride, int device = 0, unsigned flags = 0) {
    std::vector<const bn254_plonk_pvk*> h(keys.size());
    for (size_t k = 0; k < keys.size(); k++) h[k] = keys[k] ? keys[k]->handle() : nullptr;
    Bytes st(key_index.size() ? key_index.size() : 1);
    detail::check(bn254_plonk_verify_batch_keys(h.data(), h.size(), key_index.data(), proofs, stride, public_inputs, input_stride, key_index.size(), st.data(), device, flags));
    st.resize(key_index.size());
    return st;
  }
  static void reserve_keys(const std::vector<const PreparedPlonkVk*>& keys, size_t n, size_t proof_stride, int device = 0) {
    std::vector<const bn254_plonk_pvk*> h(keys.size());
    for (size_t k = 0; k < keys.size(); k++) h[k] = keys[k] ? keys[k]->handle() : nullptr;
    detail::check(bn254_plonk_reserve_keys(h.data(), h.size(), n, proof_stride, device));
  }
  // counters of the list's cached state on `device` (bn254_plonk_keys_state): passes that ran the joint check of BN254_FLAG_RLC, the groups they checked, the groups
  // that failed, passes whose per-proof pairing check ran in the cooperative form
  static std::array<uint64_t, 4> keys_state(const std::vector<const PreparedPlonkVk*>& keys, int device = 0) {
    std::vector<const bn254_plonk_pvk*> h(keys.size());
    for (size_t k = 0; k < keys.size(); k++) h[k] = keys[k] ? keys[k]->handle() : nullptr;
    std::array<uint64_t, 4> out{};
    detail::check(bn254_plonk_keys_state(h.data(), h.size(), device, out.data()));
    return out;
  }
  // passes of up to coop_max slots of a batch over a key list take the cooperative pairing form (0: always the lane form; negative: unchanged)
  static void set_keys_params(long coop_max) { bn254_set_plonk_keys_params(coop_max); }
  // the pass size from which BN254_FLAG_RLC is honoured, on one key and over a list (never below 64; negative: unchanged)
  static void set_rlc_params(long min_pass) { bn254_set_plonk_rlc_params(min_pass); }
  static Result<bool, PlonkError> outcome(uint8_t status) { return detail::plonk_outcome(status); }
};

// The known-answer self-test of the verdict kernels on `device`, now (bn254_device_selftest): an operator's health check.  The library runs it by itself before a
// device is first used (after which a device that failed makes every verification entry throw SelfTestError); this call runs it whatever ran before, and its result
// replaces the device's recorded state.  A check that disagrees is a report with passed == false; a run that could not be made throws InfrastructureError.
struct SelfTestReport {
  bool passed = false;
  unsigned failed_mask = 0;              // bit k: check k disagrees
  std::vector<std::string> failed;       // their names (bn254_selftest_check_name)
  float ms = 0.f;                        // wall time of the run
  std::string message;                   // bn254_last_error() of a failed run: the first failing check, the device's value and the expected one
};
inline SelfTestReport device_selftest(int device = 0) {
  SelfTestReport r;
  const int rc = bn254_device_selftest(device, &r.failed_mask, &r.ms);
  if (rc != BN254_OK && rc != BN254_E_SELFTEST) detail::check(rc);
  r.passed = rc == BN254_OK;
  if (!r.passed) r.message = bn254_last_error();
  for (int k = 0; k < BN254_SELFTEST_NUM_CHECKS; k++) if (r.failed_mask >> k & 1u) r.failed.push_back(bn254_selftest_check_name(k));
  return r;
}
// the recorded state of a device: -1 not run yet, 0 failed, 1 passed, 2 skipped (BN254_SELFTEST=0).  Touches no device
inline std::pair<int, unsigned> device_selftest_state(int device = 0) {
  int state = -1; unsigned mask = 0;
  detail::check(bn254_device_selftest_state(device, &state, &mask));
  return {state, mask};
}

// ---- batch pairing-product checks over caller-supplied pairs (bn254_pairing_check_batch; bn::pairing_batch of groth16/verify.rs:73-77 and plonk/kzg.rs:175-187) ------
// pairs: n items of n_pairs (1 .. 8) records G1 x | y (64 bytes), G2 x.c1 | x.c0 | y.c1 | y.c0 (128 bytes), item_stride bytes apart (0: packed, 192 * n_pairs); an
// all-zero point is the identity.  The status bytes as the header defines them; pairing_outcome maps one the way the verifiers above map theirs: true / false for
// "the product is 1 / is not", Panic for what bn's AffineG1::new / AffineG2::new turn into an error (a coordinate >= p, off the curve, outside the r-torsion).
inline bool pairing_outcome(int st) {
  if (st == BN254_ACCEPT) return true;
  if (st == BN254_REJECT) return false;
  throw Panic(st);
}
inline std::vector<uint8_t> pairing_check_batch(const Bytes& pairs, size_t n_pairs, size_t n, int device = 0, size_t item_stride = 0) {
  const size_t stride = item_stride ? item_stride : (size_t)BN254_PAIRING_PAIR_LEN * n_pairs;
  if (n && pairs.size() < (n - 1) * stride + (size_t)BN254_PAIRING_PAIR_LEN * n_pairs) throw std::invalid_argument("pairing_check_batch: the buffer is shorter than n items");
  std::vector<uint8_t> status(n);
  detail::check(bn254_pairing_check_batch(pairs.data(), stride, n_pairs, n, status.data(), device));
  return status;
}
// the final-exponentiated product of every item (384 bytes each: 12 x 32 big-endian, tower order) into *out_gt; status BN254_ACCEPT where the value is valid, else
// the loader's error
inline std::vector<uint8_t> pairing_batch(const Bytes& pairs, size_t n_pairs, size_t n, Bytes* out_gt, int device = 0, size_t item_stride = 0) {
  const size_t stride = item_stride ? item_stride : (size_t)BN254_PAIRING_PAIR_LEN * n_pairs;
  if (!out_gt) throw std::invalid_argument("pairing_batch: out_gt is null");
  if (n && pairs.size() < (n - 1) * stride + (size_t)BN254_PAIRING_PAIR_LEN * n_pairs) throw std::invalid_argument("pairing_batch: the buffer is shorter than n items");
  std::vector<uint8_t> status(n);
  out_gt->assign(384 * n, 0);
  detail::check(bn254_pairing_batch(pairs.data(), stride, n_pairs, n, out_gt->data(), status.data(), device));
  return status;
}
// ---- the same with shared, prepared G2 points (bn254_g2_prepare, bn254_pairing_check_batch_shared) ----
// The prepared record (BN254_G2_PREPARED_LEN bytes: header, affine point, 88 lines) of the G2 point x.c1 | x.c0 | y.c1 | y.c0 (128 bytes; all zero: the identity);
// Panic with BN254_ERR_NOT_MEMBER / _NOT_ON_CURVE / _NOT_IN_SUBGROUP when the point is refused.  Host work; valid only for the layout version that wrote it.
inline Bytes g2_prepare(const Bytes& g2) {
  if (g2.size() != 128) throw std::invalid_argument("g2_prepare: 128 bytes expected");
  Bytes out(BN254_G2_PREPARED_LEN);
  uint8_t st = 0;
  detail::check(bn254_g2_prepare(g2.data(), out.data(), &st));
  if (st != BN254_ACCEPT) throw Panic(st);
  return out;
}
// bytes of a packed item: BN254_PAIRING_G1_LEN per position whose bit of shared_mask is set, BN254_PAIRING_PAIR_LEN per other one
inline size_t pairing_packed_len(size_t n_pairs, unsigned shared_mask) {
  size_t len = 0;
  for (size_t j = 0; j < n_pairs; j++) len += ((shared_mask >> j) & 1u) ? (size_t)BN254_PAIRING_G1_LEN : (size_t)BN254_PAIRING_PAIR_LEN;
  return len;
}
// items: n PACKED items (a shared position holds its G1 point alone), item_stride bytes apart (0: packed); prepared: the records of the shared positions, ascending.
// The status bytes are those pairing_check_batch gives the expanded items.
inline std::vector<uint8_t> pairing_check_batch_shared(const Bytes& items, size_t n_pairs, unsigned shared_mask, const Bytes& prepared, size_t n, int device = 0, size_t item_stride = 0) {
  const size_t packed = pairing_packed_len(n_pairs, shared_mask), stride = item_stride ? item_stride : packed;
  if (n && items.size() < (n - 1) * stride + packed) throw std::invalid_argument("pairing_check_batch_shared: the buffer is shorter than n packed items");
  if (prepared.size() < (size_t)BN254_G2_PREPARED_LEN * (size_t)__builtin_popcount(shared_mask)) throw std::invalid_argument("pairing_check_batch_shared: fewer prepared records than shared positions");
  std::vector<uint8_t> status(n);
  detail::check(bn254_pairing_check_batch_shared(items.data(), stride, n_pairs, shared_mask, prepared.data(), n, status.data(), device));
  return status;
}
inline std::vector<uint8_t> pairing_batch_shared(const Bytes& items, size_t n_pairs, unsigned shared_mask, const Bytes& prepared, size_t n, Bytes* out_gt, int device = 0, size_t item_stride = 0) {
  const size_t packed = pairing_packed_len(n_pairs, shared_mask), stride = item_stride ? item_stride : packed;
  if (!out_gt) throw std::invalid_argument("pairing_batch_shared: out_gt is null");
  if (n && items.size() < (n - 1) * stride + packed) throw std::invalid_argument("pairing_batch_shared: the buffer is shorter than n packed items");
  if (prepared.size() < (size_t)BN254_G2_PREPARED_LEN * (size_t)__builtin_popcount(shared_mask)) throw std::invalid_argument("pairing_batch_shared: fewer prepared records than shared positions");
  std::vector<uint8_t> status(n);
  out_gt->assign(384 * n, 0);
  detail::check(bn254_pairing_batch_shared(items.data(), stride, n_pairs, shared_mask, prepared.data(), n, out_gt->data(), status.data(), device));
  return status;
}
// makes `device` ready for batches of n items: a later bn254_pairing_check_batch_device of up to n items only enqueues
inline void pairing_reserve(size_t n, int device = 0) { detail::check(bn254_pairing_reserve(n, device)); }
// pairing_check_batch_shared with a flags word (bn254_pairing_check_batch_flags): flags may hold BN254_FLAG_RLC only, 0 is the exact entry, shared_mask 0 with empty
// `prepared` the all-variable item.  With the flag honoured (launches of pairing_rlc_params() items or more of a shape WITHOUT a variable position; any other launch is the exact one) the 64 items of a wavefront are checked jointly under fresh
// random weights: the statuses of the exact entry except that a false ACCEPT has probability about 2^-127 per item; the call synchronises once per launch
inline std::vector<uint8_t> pairing_check_batch_flags(const Bytes& items, size_t n_pairs, unsigned shared_mask, const Bytes& prepared, size_t n, unsigned flags, int device = 0,
                                                      size_t item_stride = 0) {
  if (n_pairs < 1 || n_pairs > (size_t)BN254_PAIRING_MAX_PAIRS || (shared_mask >> n_pairs)) throw std::invalid_argument("pairing_check_batch_flags: n_pairs is 1 .. 8 and shared_mask has bits below n_pairs only");
  size_t packed = 0;
  for (size_t j = 0; j < n_pairs; j++) packed += ((shared_mask >> j) & 1u) ? (size_t)BN254_PAIRING_G1_LEN : (size_t)BN254_PAIRING_PAIR_LEN;
  const size_t stride = item_stride ? item_stride : packed;
  if (n && (stride < packed || items.size() < (n - 1) * stride + packed)) throw std::invalid_argument("pairing_check_batch_flags: the buffer is shorter than n packed items");
  if (prepared.size() < (size_t)BN254_G2_PREPARED_LEN * (size_t)__builtin_popcount(shared_mask)) throw std::invalid_argument("pairing_check_batch_flags: fewer prepared records than shared positions");
  std::vector<uint8_t> status(n);
  detail::check(bn254_pairing_check_batch_flags(items.data(), stride, n_pairs, shared_mask, shared_mask ? prepared.data() : nullptr, n, status.data(), device, flags));
  return status;
}
// enqueues on hip_stream; a launch that honours BN254_FLAG_RLC synchronises it once
inline void pairing_check_batch_flags_device(const void* d_items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const void* d_prepared, size_t n, void* d_status,
                                             unsigned flags, int device = 0, void* hip_stream = nullptr) {
  detail::check(bn254_pairing_check_batch_flags_device(d_items, item_stride, n_pairs, shared_mask, d_prepared, n, d_status, device, hip_stream, flags));
}
// BN254_FLAG_RLC on the pairing batch is honoured from rlc_min items per launch on (never below 64; negative: unchanged)
inline void set_pairing_rlc_params(long rlc_min) { bn254_set_pairing_rlc_params(rlc_min); }
inline long pairing_rlc_params() { long out[1] = {0}; detail::check(bn254_pairing_rlc_params(out)); return out[0]; }
// {launches that ran the joint check, groups they checked, groups that failed, launches on the exact path}
inline std::array<uint64_t, 4> pairing_rlc_state() { std::array<uint64_t, 4> out{}; detail::check(bn254_pairing_rlc_state(out.data())); return out; }
// launches of up to coop_max items take the cooperative twelve-lane form (0: always the lane form; clamped to 30 720; negative: unchanged) / the knob as it is now
inline void set_pairing_params(long coop_max) { bn254_set_pairing_params(coop_max); }
inline long pairing_params() { long out[1] = {0}; detail::check(bn254_pairing_params(out)); return out[0]; }
// launches enqueued so far by this process: {in the cooperative form, in the lane form}
inline std::array<uint64_t, 2> pairing_state() { std::array<uint64_t, 2> out{}; detail::check(bn254_pairing_state(out.data())); return out; }

// ---- batch verification of KZG openings (bn254_kzg_key_prepare, bn254_kzg_verify_batch) ----
// The key is plain data (BN254_KZG_KEY_LEN bytes: header, g1, the prepared records of g2 and tau_g2): no handle, no per-device state.  prepare: Panic with the first
// failure over g1 (64 bytes), g2, tau_g2 (128 bytes each) when a point is refused.  verify_batch: n openings C | H | z | y (BN254_KZG_OPENING_LEN bytes), stride bytes
// apart (0: packed); status[i] is BN254_ACCEPT where e(C - y g1 + z H, g2) e(-H, tau_g2) == 1, BN254_REJECT where it is not, or the loader error.  flags:
// BN254_FLAG_STRICT_SCALARS, BN254_FLAG_RLC (the joint check over groups of 64 openings, honoured from set_kzg_params' rlc_min openings per launch on)
class KzgVerifier {
 public:
  static KzgVerifier prepare(const Bytes& g1, const Bytes& g2, const Bytes& tau_g2) {
    if (g1.size() != 64 || g2.size() != 128 || tau_g2.size() != 128) throw std::invalid_argument("KzgVerifier::prepare: 64, 128 and 128 bytes expected");
    KzgVerifier v;
    v.key_.resize(BN254_KZG_KEY_LEN);
    uint8_t st = 0;
    detail::check(bn254_kzg_key_prepare(g1.data(), g2.data(), tau_g2.data(), v.key_.data(), &st));
    if (st != BN254_ACCEPT) throw Panic(st);
    return v;
  }
  const Bytes& key() const { return key_; }      // for a caller that keeps the openings on the device (bn254_kzg_verify_batch_device)
  std::vector<uint8_t> verify_batch(const Bytes& openings, size_t n, int device = 0, unsigned flags = 0, size_t stride = 0) const {
    const size_t s = stride ? stride : (size_t)BN254_KZG_OPENING_LEN;
    if (n && (s < (size_t)BN254_KZG_OPENING_LEN || openings.size() < (n - 1) * s + BN254_KZG_OPENING_LEN)) throw std::invalid_argument("KzgVerifier::verify_batch: the buffer is shorter than n openings");
    std::vector<uint8_t> status(n);
    detail::check(bn254_kzg_verify_batch(key_.data(), openings.data(), s, n, status.data(), device, flags));
    return status;
  }
  // makes `device` ready for batches of n openings: a later bn254_kzg_verify_batch_device of up to n openings without BN254_FLAG_RLC only enqueues
  static void reserve(size_t n, int device = 0) { detail::check(bn254_kzg_reserve(n, device)); }
  // batch-opening proofs (bn254_kzg_verify_folded_batch): n records of n_digests digests and data_len bytes of caller data each, BN254_KZG_FOLD_LEN(n_digests,
  // data_len) bytes, stride bytes apart (0: packed): D_0 .. D_{k-1} | H | z | y_0 .. y_{k-1} | data.  status[i] is BN254_ACCEPT where the digests folded with the
  // transcript's gamma open to the folded values, BN254_REJECT where they do not, or the loader error; flags as verify_batch
  std::vector<uint8_t> verify_folded_batch(const Bytes& records, size_t n, size_t n_digests, size_t data_len = 0, int device = 0, unsigned flags = 0, size_t stride = 0) const {
    if (n_digests < 1 || n_digests > (size_t)BN254_KZG_FOLD_MAX_DIGESTS || data_len > (size_t)BN254_KZG_FOLD_MAX_DATA)
      throw std::invalid_argument("KzgVerifier::verify_folded_batch: n_digests is 1 .. BN254_KZG_FOLD_MAX_DIGESTS, data_len at most BN254_KZG_FOLD_MAX_DATA");
    const size_t len = BN254_KZG_FOLD_LEN(n_digests, data_len), s = stride ? stride : len;
    if (n && (s < len || records.size() < (n - 1) * s + len)) throw std::invalid_argument("KzgVerifier::verify_folded_batch: the buffer is shorter than n records");
    std::vector<uint8_t> status(n);
    detail::check(bn254_kzg_verify_folded_batch(key_.data(), records.data(), s, n, n_digests, data_len, status.data(), device, flags));
    return status;
  }
  // ... a later bn254_kzg_verify_folded_batch_device of up to n records of n_digests digests without BN254_FLAG_RLC only enqueues
  static void reserve_folded(size_t n, size_t n_digests, int device = 0) { detail::check(bn254_kzg_fold_reserve(n, n_digests, device)); }

 private:
  Bytes key_;
};
// BN254_FLAG_RLC is honoured from rlc_min openings per launch on (never below 64; negative: unchanged) / the knob as it is now
inline void set_kzg_params(long rlc_min) { bn254_set_kzg_params(rlc_min); }
inline long kzg_params() { long out[1] = {0}; detail::check(bn254_kzg_params(out)); return out[0]; }
// {launches that ran the joint check, groups they checked, groups that failed, launches on the exact path}
inline std::array<uint64_t, 4> kzg_state() { std::array<uint64_t, 4> out{}; detail::check(bn254_kzg_state(out.data())); return out; }

// ---- batch G1 multi-scalar multiplication with per-item and shared bases (bn254_g1_bases_prepare, bn254_g1_msm_batch) ----
// An item is n_var pairs (point x | y, scalar), n_unit points, n_shared scalars for the shared bases: BN254_G1_MSM_ITEM_LEN(n_var, n_unit, n_shared) bytes, 32-byte
// big-endian fields.  G1Bases owns the window tables of 1 .. BN254_G1_MSM_MAX_SHARED points on one device: prepare throws Panic with the first failure over the points;
// the destructor waits for the device and frees them.  msm_batch: per item the 64 bytes of sum k_t P_t + sum U_t + sum c_j B_j (zero: the identity, or an item that
// ended in an error) and status[i], BN254_ACCEPT or the loader error.  flags: BN254_FLAG_STRICT_SCALARS
inline size_t g1_msm_item_len(size_t n_var, size_t n_unit, size_t n_shared) { return BN254_G1_MSM_ITEM_LEN(n_var, n_unit, n_shared); }
class G1Bases {
 public:
  static G1Bases prepare(const Bytes& points, int device = 0) {
    if (points.empty() || points.size() % 64 || points.size() / 64 > (size_t)BN254_G1_MSM_MAX_SHARED) throw std::invalid_argument("G1Bases::prepare: 1 .. BN254_G1_MSM_MAX_SHARED points of 64 bytes");
    G1Bases b;
    uint8_t st = 0;
    detail::check(bn254_g1_bases_prepare(points.data(), points.size() / 64, device, &b.h_, &st));
    if (st != BN254_ACCEPT || !b.h_) throw Panic(st);
    b.device_ = device;
    return b;
  }
  G1Bases(G1Bases&& o) noexcept : h_(o.h_), device_(o.device_) { o.h_ = nullptr; }
  G1Bases& operator=(G1Bases&& o) noexcept { if (this != &o) { bn254_g1_bases_free(h_); h_ = o.h_; device_ = o.device_; o.h_ = nullptr; } return *this; }
  G1Bases(const G1Bases&) = delete;
  G1Bases& operator=(const G1Bases&) = delete;
  ~G1Bases() { bn254_g1_bases_free(h_); }
  const void* handle() const { return h_; }      // for a caller that keeps the items on the device (bn254_g1_msm_batch_device)
  size_t size() const { return bn254_g1_bases_count(h_); }
  int device() const { return device_; }

 private:
  G1Bases() = default;
  void* h_ = nullptr; int device_ = 0;
};
struct G1MsmResult { Bytes out; std::vector<uint8_t> status; };      // 64 bytes x | y and a status byte per item
inline G1MsmResult g1_msm_batch(const Bytes& items, size_t n, size_t n_var, size_t n_unit, size_t n_shared, const G1Bases* bases = nullptr, int device = 0, unsigned flags = 0,
                                size_t stride = 0) {
  const size_t len = g1_msm_item_len(n_var, n_unit, n_shared), s = stride ? stride : len;
  if (n && (s < len || items.size() < (n - 1) * s + len)) throw std::invalid_argument("g1_msm_batch: the buffer is shorter than n items");
  G1MsmResult r;
  r.out.resize(64 * n); r.status.resize(n);
  detail::check(bn254_g1_msm_batch(items.data(), s, n_var, n_unit, n_shared, bases ? bases->handle() : nullptr, n, r.out.data(), r.status.data(), device, flags));
  return r;
}
// enqueues on hip_stream and returns: d_out receives 64 n bytes, d_status n
inline void g1_msm_batch_device(const void* d_items, size_t n, size_t n_var, size_t n_unit, size_t n_shared, const G1Bases* bases, void* d_out, void* d_status, int device = 0,
                                void* hip_stream = nullptr, unsigned flags = 0, size_t stride = 0) {
  detail::check(bn254_g1_msm_batch_device(d_items, stride ? stride : g1_msm_item_len(n_var, n_unit, n_shared), n_var, n_unit, n_shared, bases ? bases->handle() : nullptr, n, d_out,
                                          d_status, device, hip_stream, flags));
}
// makes `device` ready for batches of n items of this shape: a later g1_msm_batch_device of up to n such items only enqueues
inline void g1_msm_reserve(size_t n, size_t n_var, size_t n_unit, size_t n_shared, int device = 0) { detail::check(bn254_g1_msm_reserve(n, n_var, n_unit, n_shared, device)); }

}  // namespace snark_bn254_verifier
