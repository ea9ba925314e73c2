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

// ---- PlonK batches over many keys (bn254_plonk_verify_batch_keys, bn254_capi_plonk_keys.hip) ------------------------------------------------------------------------
// The same slots and granules.  What a kernel of a PlonK pass reads about entry k of the list: the parsed key of the stage kernels, the window tables of its points
// (k_g1_msm_rows_keys), the line tables of its two KZG G2 points (k_miller_run_fixed2_keys).  All four are the member's OWN per-device state (PlonkDev).
#define PLONK_KEYS_MAX_KEYS 256u
struct PlonkKeyDesc {
  const void* key;             // PlonkKey (bn254_plonk.hpp)
  const int32_t* fixed_tabs;   // plonk_num_tables x MSM_FW_WINDOWS x MSM_FW_ENTRIES entries
  const int32_t* tab0;         // BN_ATE_STEPS * FIXED_LINE_DWORDS: lines of kzg_g2[0]
  const int32_t* tab1;         // the same for kzg_g2[1]
  uint32_t n_public;           // the key's nb_public: the width of its proofs' input rows
  uint32_t pad_;
};
#if defined(__HIPCC__)
// The descriptor of the granule that starts at slot wave_first of the launch, read through the constant address space with a readfirstlane'd index (scalar loads;
// bn254_devws.h::keys_view has the measurement of what generic pointers cost).  fixed_tabs is read at per-lane addresses: global address space.
struct PlonkKeyView { const void* key; const int32_t *fixed_tabs, *tab0, *tab1; uint32_t n_public; };
__device__ __forceinline__ PlonkKeyView plonk_keys_view(const PlonkKeyDesc* __restrict__ desc, const uint32_t* __restrict__ granule_key, uint32_t wave_first, uint32_t n_keys) {
  static_assert(sizeof(PlonkKeyDesc) == 40, "four pointers and two words");
  typedef const __attribute__((address_space(4))) uint64_t* cptr64;
  uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)granule_key[wave_first / G16_KEYS_GRANULE]);
  k = k < n_keys ? k : 0u;
  const uint64_t b = (uint64_t)(desc + k);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  cptr64 f = (cptr64)(((uint64_t)hi << 32) | lo);
  auto cst = [](uint64_t bits) {
    const uint32_t l = __builtin_amdgcn_readfirstlane((uint32_t)bits), h = __builtin_amdgcn_readfirstlane((uint32_t)(bits >> 32));
    return (const int32_t*)(const __attribute__((address_space(4))) int32_t*)(((uint64_t)h << 32) | l);
  };
  PlonkKeyView v;
  v.key = (const void*)cst(f[0]);
  v.fixed_tabs = (const int32_t*)(const __attribute__((address_space(1))) int32_t*)f[1];
  v.tab0 = cst(f[2]); v.tab1 = cst(f[3]);
  v.n_public = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)f[4]);
  return v;
}
#endif

}  // namespace bn254
