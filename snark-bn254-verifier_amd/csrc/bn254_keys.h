// bn254_keys.h -- Groth16 batches over many verifying keys (bn254_groth16_verify_batch_keys): how the proofs of a mixed batch are brought into SLOTS so that every
// granule of G16_KEYS_GRANULE consecutive slots holds proofs of one key, and what a kernel reads about a key.  The arithmetic of the three grouping steps (count,
// scan, place) is here once, for the kernels of bn254_k_keys.hip and for the host (bn254_dbg_g16_keys_group with device -1, the CPU tests), the way bn254_sha256.h and
// bn254_codec.h serve both sides.  Depends on nothing but <stdint.h>.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KEYS_HD __host__ __device__ inline
#else
#define KEYS_HD inline
#endif

namespace bn254 {

// A granule is one wavefront: the line tables are read with wavefront-uniform scalar loads, k_g16_prepare_keys stages its records per wavefront, and the parking space
// of the Miller kernel is lane-private, so nothing needs a key to be constant over more than 64 lanes.  Padding is at most 63 slots per key that has proofs (a
// workgroup-sized granule would make it 255: at 4096 keys and 65 536 proofs up to 16 x the proofs instead of 4 x).
#define G16_KEYS_GRANULE 64u
#define G16_KEYS_MAX_KEYS 65536u       // entries of a key list
#define G16_KEYS_MAX_PUBLIC 16u        // keys with more public inputs run the wide / comb MSM kernels: a different pipeline, not in a set
#define G16_KEYS_NO_PROOF 0xffffffffu  // slot -> proof index of a padding slot

// what the kernels read about entry k of the key list: one array per (set, device), read with scalar loads (the index is wavefront-uniform)
struct G16KeyDesc {
  const int32_t* msm_tab;   // byte-window tables of K[1..]: n_public * 32 * 255 entries of MSM_ENTRY_DWORDS (bn254_k_comb.hip form 1)
  const int32_t* k0;        // 18 dwords: affine K[0]
  const int32_t* gtab;      // BN_ATE_STEPS * FIXED_LINE_DWORDS: lines of the G2 argument paired with L
  const int32_t* dtab;      // the same for the one paired with C
  const int32_t* target;    // 108 dwords: e(alpha, beta)
  int32_t n_public;         // len(vk.K) - 1 (0 for a key without K points)
  int32_t inputs_match;     // 0 for a key without K points: every proof that loads answers INPUT_LEN
};

KEYS_HD uint32_t keys_round_up(uint32_t count) { return (count + (G16_KEYS_GRANULE - 1u)) & ~(G16_KEYS_GRANULE - 1u); }
// Slots a batch of n proofs over n_keys keys can need at most: every key that has proofs pads its run to a whole granule, and the total is a whole number of granules.
// This is what the workspace of a reservation is sized for and what a launch covers when the real figure is only known on the device.
KEYS_HD uint64_t keys_slot_bound(uint64_t n, uint64_t n_keys) {
  const uint64_t k = n_keys < n ? n_keys : n;
  return (n + k * (G16_KEYS_GRANULE - 1u)) / G16_KEYS_GRANULE * G16_KEYS_GRANULE;
}
// scan step over keys [lo, hi): base[k] = first slot of key k's run given the slots before lo; returns the slots after hi - 1
KEYS_HD uint32_t keys_scan_range(const uint32_t* count, uint32_t* base, uint32_t lo, uint32_t hi, uint32_t before) {
  for (uint32_t k = lo; k < hi; k++) { base[k] = before; before += keys_round_up(count[k]); }
  return before;
}
// place step: proof i of key k got position pos (base[k] + its rank among the key's proofs, in any order)
KEYS_HD void keys_place(uint32_t* slot_to_proof, uint32_t* granule_key, uint32_t pos, uint32_t i, uint32_t k) {
  slot_to_proof[pos] = i;
  if ((pos & (G16_KEYS_GRANULE - 1u)) == 0) granule_key[pos / G16_KEYS_GRANULE] = k;   // every granule of a run holds at least the proof in its first slot
}

// The three steps on the host, one after the other.  slot_to_proof: keys_slot_bound(n, n_keys) words, granule_key: a word per granule of them, count / base: n_keys words
// of scratch.  Returns the number of slots; an index >= n_keys gets no slot (the entries refuse such a batch or answer MALFORMED for the proof).
inline uint32_t keys_group_host(const uint32_t* key_index, uint32_t n, uint32_t n_keys, uint32_t* slot_to_proof, uint32_t* granule_key, uint32_t* count, uint32_t* base) {
  for (uint32_t k = 0; k < n_keys; k++) count[k] = 0;
  for (uint32_t i = 0; i < n; i++) if (key_index[i] < n_keys) count[key_index[i]]++;
  const uint32_t n_slots = keys_scan_range(count, base, 0, n_keys, 0);
  for (uint32_t s = 0; s < n_slots; s++) slot_to_proof[s] = G16_KEYS_NO_PROOF;
  for (uint32_t i = 0; i < n; i++) if (key_index[i] < n_keys) keys_place(slot_to_proof, granule_key, base[key_index[i]]++, i, key_index[i]);
  return n_slots;
}

}  // namespace bn254
