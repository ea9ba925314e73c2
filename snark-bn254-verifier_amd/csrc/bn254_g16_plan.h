// bn254_g16_plan.h -- how a Groth16 batch is cut into workspace chunks, sub-batches (parts) and launch forms, and what a (key, device) context allocates
// for a reservation: PURE functions of the sizes, shared by the code that allocates (bn254_capi.hip::ensure_dev), the code that enqueues
// (g16_enqueue_exact, bn254_launch_g16) and the probe tests/test_capi_cpu.py reads through bn254_dbg_g16_plan.  The launch form of a batch follows the
// BATCH's size, the buffers the RESERVATION's: the property test walks batch sizes against reservations and asserts that every launch fits (the class of
// the PlonK scratch overflow of round 3, found there by a sweep instead of a test).  BN254_FLAG_RLC has a chunk plan of its own, G16RlcChunkPlan, shared in the
// same way by rlc_ensure, g16_enqueue_rlc and the probes bn254_dbg_g16_rlc_plan / bn254_dbg_g16_rlc_wide_plan.  (Whether a chunk's sub-batches run side by side
// at all is decided from measurements: bn254_overlap_vote.h.)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "bn254_kernels.h"

namespace bn254 {

// ---- what ensure_dev allocates for a reservation of n proofs against a key with `key_inputs` public inputs ------------------------------------------------
struct G16Alloc {
  size_t ws_proofs;          // proofs the workspace holds (G16_WS_BYTES_PER_PROOF each)
  size_t msm_part_proofs;    // keys with many inputs: proofs the partial-sum / digit buffer holds per launch (0: the key has none)
  size_t msm_chunks;         // partial sums per proof
  size_t msm_part_bytes;     // chunks * 27 dwords * proofs
  size_t msm_digit_bytes;    // comb tables: G16_COMB_COLS * key_inputs * proofs u16
};
inline size_t g16_round256(size_t n) { return (n + 255) / 256 * 256; }
inline G16Alloc g16_alloc_for(size_t n, size_t key_inputs, bool comb) {
  G16Alloc a = {0, 0, 0, 0, 0};
  a.ws_proofs = g16_round256(n) < (size_t)G16_MAX_BATCH ? g16_round256(n) : (size_t)G16_MAX_BATCH;   // larger batches run in chunks of G16_MAX_BATCH
  if (key_inputs > (size_t)G16_WIDE_MSM_MIN_INPUTS) {
    a.msm_part_proofs = n < (size_t)G16_WIDE_MSM_MAX_PROOFS ? g16_round256(n) : (size_t)G16_WIDE_MSM_MAX_PROOFS;
    a.msm_chunks = (key_inputs + G16_WIDE_MSM_INPUTS_PER_LANE - 1) / G16_WIDE_MSM_INPUTS_PER_LANE;
    a.msm_part_bytes = a.msm_chunks * 27 * a.msm_part_proofs * sizeof(int32_t);
    a.msm_digit_bytes = comb ? (size_t)G16_COMB_COLS * key_inputs * a.msm_part_proofs * sizeof(uint16_t) : 0;
  }
  return a;
}

// ---- the form of ONE launch (bn254_launch_g16) --------------------------------------------------------------------------------------------------------------
enum { G16_FORM_LANES = 0, G16_FORM_COOP = 1, G16_FORM_LATENCY = 2 };
struct G16Form {
  int form;          // cooperative kernels (twelve lanes per proof), lane kernels, or the lane kernels' latency mode (three Miller chains on three streams)
  int run_steps;     // lane kernels: Miller steps per k_miller_run launch (0: one launch per step)
  bool wide;         // the public-input MSM runs as (proof, chunk) lanes through the partial-sum buffer
};
// n: proofs of the launch; n_public: inputs per proof AS PASSED; inputs_match_key: n_public + 1 == len(vk.K); has_msm_part: the caller handed a partial-sum buffer;
// part_of_larger: one of several sub-batches; have_split_streams: the caller provided the two extra streams of the latency mode
inline G16Form g16_launch_form(size_t n, size_t n_public, bool inputs_match_key, bool has_msm_part, bool part_of_larger, bool have_split_streams, bool coop_on, int run_steps_env) {
  G16Form f;
  f.wide = has_msm_part && inputs_match_key && n_public > (size_t)G16_WIDE_MSM_MIN_INPUTS;
  const bool coop = coop_on && !part_of_larger && n <= (size_t)COOP12_MAX_PROOFS && (f.wide || n_public <= (size_t)G16_WIDE_MSM_MIN_INPUTS);
  f.form = coop ? G16_FORM_COOP : (have_split_streams && n <= (size_t)G16_SPLIT_MAX_PROOFS) ? G16_FORM_LATENCY : G16_FORM_LANES;
  // steps of the Miller loop per launch: a batch that is ONE sub-batch takes the whole loop; sub-batches of a larger batch that are a single generation of
  // workgroups run better in a few shorter launches (profiles/r03_run_steps_sweep.txt)
  f.run_steps = run_steps_env >= 0 ? run_steps_env : !part_of_larger ? 88 : (n <= 65536 ? 11 : n <= 131072 ? 22 : n <= 262144 ? 44 : 88);
  return f;
}

// ---- the reduction of a wide launch (bn254_launch_g16_loader) -------------------------------------------------------------------------------------------------
// inputs per lane of the partial sums (wide_per_knob: knob_wide_per(), 0 = the default), the chunk sums per proof that follow, and which kernel adds them up: eight
// lanes per proof (k_g16_msm_reduce8) from 16 chunks on while the launch is at most one wavefront per SIMD, one lane's chain (k_g16_msm_reduce) otherwise
inline int g16_wide_per(int wide_per_knob) { return wide_per_knob ? wide_per_knob : G16_WIDE_MSM_INPUTS_PER_LANE; }
inline int g16_wide_chunks(size_t n_public, int per) { return (int)((n_public + (size_t)per - 1) / (size_t)per); }
inline bool g16_wide_reduce8(size_t chunks, size_t n) { return chunks >= 16 && n <= 65536; }

// ---- the launch knobs of the environment ------------------------------------------------------------------------------------------------------------------
// BN254_COOP, BN254_MILLER_RUN_STEPS, BN254_COOP_FIXED_MAX and BN254_WIDE_PER are read ONCE per process, here and nowhere else, as raw values (set_*: the variable
// is there at all).  What a value means is each launcher's own rule: the one-line functions below, side by side.  bn254_dbg_launch_knobs shows them as the process
// sees them.
#define G16_MILLER_STEPS 88   // BN_ATE_STEPS (bn254_constants.h; static_asserted in bn254_kernels.hip)
struct LaunchKnobs { bool set_coop, set_run_steps, set_coop_fixed_max, set_wide_per; int coop, run_steps, wide_per; long coop_fixed_max; bool set_kzg_rlc_min; long kzg_rlc_min; bool set_g1_msm_pass; long g1_msm_pass; };
inline const LaunchKnobs& launch_knobs() {
  static const LaunchKnobs knobs = [] {
    LaunchKnobs k = {false, false, false, false, 0, 0, 0, 0, false, 0, false, 0};
    if (const char* e = getenv("BN254_COOP")) { k.set_coop = true; k.coop = atoi(e); }
    if (const char* e = getenv("BN254_MILLER_RUN_STEPS")) { k.set_run_steps = true; k.run_steps = atoi(e); }
    if (const char* e = getenv("BN254_COOP_FIXED_MAX")) { k.set_coop_fixed_max = true; k.coop_fixed_max = atol(e); }
    if (const char* e = getenv("BN254_WIDE_PER")) { k.set_wide_per = true; k.wide_per = atoi(e); }
    if (const char* e = getenv("BN254_KZG_RLC_MIN")) { k.set_kzg_rlc_min = true; k.kzg_rlc_min = atol(e); }
    if (const char* e = getenv("BN254_G1_MSM_PASS")) { k.set_g1_msm_pass = true; k.g1_msm_pass = atol(e); }
    return k;
  }();
  return knobs;
}
// BN254_COOP=0 switches every cooperative form off: the lane kernels at every size
inline bool knob_coop_on() { const LaunchKnobs& k = launch_knobs(); return !k.set_coop || k.coop != 0; }
// BN254_MILLER_RUN_STEPS, Groth16: the steps per k_miller_run launch handed to g16_launch_form; -1: the plan's own choice
//   bn254_launch_g16: 0 selects the one-launch-per-step kernels (k_miller_step_dbl / _add, with k_vm_init, k_g16_subgroup and k_g16_compare as launches of their own)
inline int knob_run_steps_g16() { const LaunchKnobs& k = launch_knobs(); return !k.set_run_steps || k.run_steps < -1 ? -1 : k.run_steps; }
//   bn254_launch_g16_keys: only k_miller_run_keys reads the key per wavefront, so 0 is the plan's choice too
inline int knob_run_steps_g16_keys() { const LaunchKnobs& k = launch_knobs(); return !k.set_run_steps || k.run_steps < 1 ? -1 : k.run_steps; }
// BN254_MILLER_RUN_STEPS, PlonK's two-pair check: the steps per k_miller_run_fixed2 launch; by default the whole loop
//   bn254_launch_pairing2_fixed_lanes: 0 selects one launch per operation (k_f12_sqr, k_f12_mul_line_fixed2)
inline int knob_run_steps_pairing2_lanes() { const LaunchKnobs& k = launch_knobs(); return !k.set_run_steps || k.run_steps < 0 ? G16_MILLER_STEPS : k.run_steps; }
//   bn254_launch_pairing2_fixed_keys: the one-launch-per-operation kernels read one key per launch, so 0 is the whole loop too
inline int knob_run_steps_pairing2_keys() { const LaunchKnobs& k = launch_knobs(); return !k.set_run_steps || k.run_steps <= 0 ? G16_MILLER_STEPS : k.run_steps; }
//   bn254_launch_pairing_batch: k_miller_run_var is the only form of the variable-pair loop, so 0 is the whole loop too
inline int knob_run_steps_pairing_batch() { const LaunchKnobs& k = launch_knobs(); return !k.set_run_steps || k.run_steps <= 0 ? G16_MILLER_STEPS : k.run_steps; }
// BN254_COOP_FIXED_MAX: the largest two-pair check that takes the cooperative kernel (bn254_launch_pairing2_fixed)
inline size_t knob_coop_fixed_max() { const LaunchKnobs& k = launch_knobs(); return k.set_coop_fixed_max ? (size_t)k.coop_fixed_max : (size_t)COOP12_MAX_PROOFS_FIXED; }
// BN254_WIDE_PER (experiments): inputs per lane of the wide MSM, at least G16_WIDE_MSM_INPUTS_PER_LANE (the partial-sum buffer is sized for that many chunks); 0: the default
inline int knob_wide_per() { const LaunchKnobs& k = launch_knobs(); return k.set_wide_per && k.wide_per >= G16_WIDE_MSM_INPUTS_PER_LANE && k.wide_per <= 256 ? k.wide_per : 0; }
// BN254_KZG_RLC_MIN: the initial value of bn254_set_kzg_params (bn254_capi_kzg.hip clamps it); -1: not set
inline long knob_kzg_rlc_min() { const LaunchKnobs& k = launch_knobs(); return k.set_kzg_rlc_min && k.kzg_rlc_min >= 0 ? k.kzg_rlc_min : -1; }
// BN254_G1_MSM_PASS (tests): lowers the items per pass of bn254_g1_msm_batch, 64 at least (bn254_capi_g1msm.hip); 0: not set
inline size_t knob_g1_msm_pass() { const LaunchKnobs& k = launch_knobs(); return !k.set_g1_msm_pass ? 0 : k.g1_msm_pass < 64 ? (size_t)64 : (size_t)k.g1_msm_pass; }

// ---- compaction of a lane launch (k_g16_classify / k_g16_compact_write, bn254_k_g16_load.hip) ----------------------------------------------
// A proof the loader decides for good (a coordinate >= p, A or B off the curve) would still ride its wavefront through the Miller loop and the final
// exponentiation.  A launch that compacts classifies first and runs k_g16_prepare and everything after it on the dense, order-preserving list of the proofs
// still pending: slot j of the launch holds proof slot_proof[j], and the wavefronts past the list see slot status 0 and leave in their prologue.
// Which launches: the lane form with the Miller loop as k_miller_run launches (the tail of the loop resolves a slot's status in place, and the verdict product, the
// last launch, hands every slot's final byte to its proof through slot_proof), a key whose input sum runs inside k_g16_prepare, neither BN254_FLAG_STRICT_SCALARS
// nor the RLC mode (its exact second pass included).  The cooperative kernels, the latency mode, wide keys and batches over many keys run as they always did.
#define G16_COMPACT_BLOCK 256
#define G16_COMPACT_NO_PROOF 0xffffffffu
// the key's half of the predicate: its input sum runs inside k_g16_prepare.  What the allocator asks (a context of such a key holds the slot arrays) and what every call asks
inline bool g16_key_may_compact(size_t key_inputs) { return key_inputs <= (size_t)G16_WIDE_MSM_MIN_INPUTS; }
inline bool g16_compacts(const G16Form& f, size_t key_inputs, bool strict_scalars, bool rlc) {
  return g16_key_may_compact(key_inputs) && f.form == G16_FORM_LANES && f.run_steps > 0 && !f.wide && !strict_scalars && !rlc;
}
// what ensure_dev allocates beside a workspace of ws_proofs proofs (a multiple of 256): slot_proof (4 B per slot), slot_status (1 B per slot) and one count of
// pending proofs per block of 256.  A part of a chunk addresses them at its first proof (a multiple of 256), as it addresses the workspace.
struct G16CompactAlloc { size_t slot_proof_bytes, slot_status_bytes, count_bytes; };
inline G16CompactAlloc g16_compact_alloc(size_t ws_proofs, size_t key_inputs) {
  G16CompactAlloc a = {0, 0, 0};
  if (!g16_key_may_compact(key_inputs)) return a;
  a.slot_proof_bytes = ws_proofs * sizeof(uint32_t); a.slot_status_bytes = ws_proofs;
  a.count_bytes = (ws_proofs + G16_COMPACT_BLOCK - 1) / G16_COMPACT_BLOCK * sizeof(uint32_t);
  return a;
}
// The scan step, shared by k_g16_compact_write and its host restatement (bn254_dbg_g16_compact): lane t of 256 sums the counts t, t + 256, ... below `block` into
// *before and all of them into *total; the caller adds the 256 pairs up.  At most G16_MAX_LAUNCH / 256 = 3072 counts: twelve per lane.
static inline __host__ __device__ void g16_compact_partial(const uint32_t* count, uint32_t blocks, uint32_t block, uint32_t t, uint32_t* before, uint32_t* total) {
  uint32_t b = 0, a = 0;
  for (uint32_t k = t; k < blocks; k += G16_COMPACT_BLOCK) { const uint32_t c = count[k]; a += c; if (k < block) b += c; }
  *before = b; *total = a;
}

// ---- the form of a batch over many keys (bn254_groth16_verify_batch_keys[_device]) ---------------------------------------------------------------------------
// From n alone: both entries know it on the host, the device entry does not know the slot count.  Up to keys_coop_max proofs (bn254_set_keys_params; never with
// BN254_COOP=0) the DIRECT form: a slot is a proof, k_g16_prepare + k_coop12_miller_g16_keys, no grouping launches.  Otherwise the grouped lane form on
// keys_slot_bound(n, n_keys) slots at most.
enum { G16_KEYS_FORM_GROUPED = 0, G16_KEYS_FORM_DIRECT = 1 };
// the hand-over: the largest measured n at which the direct form beats the grouped one (the parent revision's library) by more than the two cells' spreads at EVERY key
// count measured: 30 720, the largest size measured -- 11.69 against 12.54 ms with one key, 12.10 against 42.15 ms with 4096 (profiles/r10_multikey_small.txt;
// DESIGN.md section 9d)
#define G16_KEYS_COOP_MAX_DEFAULT COOP12_MAX_PROOFS
inline int g16_keys_form(size_t n, size_t keys_coop_max, bool coop_on) { return coop_on && n <= keys_coop_max && n <= (size_t)COOP12_MAX_PROOFS ? G16_KEYS_FORM_DIRECT : G16_KEYS_FORM_GROUPED; }

// ---- the form of ONE launch of the batch pairing product (bn254_launch_pairing_batch) ---------------------------------------------------------------------------
// Up to coop_max items (bn254_set_pairing_params; never with BN254_COOP=0, never above the cooperative kernels' range) the cooperative form: k_pairing_load, then
// k_coop12_miller_pairs, twelve lanes per item.  Otherwise the lane form, one item per lane.  A launch takes one form whole.  The rule is n <= coop_max, not
// n * n_pairs <= coop_max, because that is what was measured (profiles/r15_pairing_coop.txt): with both forms alternating in one session at
// n in {1, 256, 1024, 4096, 8192, 16 384, 30 720} and 1, 2, 3, 4, 8 pairs, the largest size at which the cooperative median is not above the lane median is 16 384 at
// EVERY pair count (8 pairs: 24.3 against 31.9 ms there, 35.9 against 32.1 ms at 30 720; 1 pair: 6.30 against 9.05 and 9.22 against 9.18) -- the default.
enum { PAIRING_FORM_PLAN = 0, PAIRING_FORM_LANES = 1, PAIRING_FORM_COOP = 2 };
#define PAIRING_COOP_MAX_DEFAULT 16384
inline int pairing_form(size_t n_pairs, size_t n, size_t coop_max, bool coop_on) {
  (void)n_pairs;
  return coop_on && n <= coop_max && n <= (size_t)COOP12_MAX_PROOFS ? PAIRING_FORM_COOP : PAIRING_FORM_LANES;
}

// ---- one workspace chunk (at most G16_MAX_BATCH proofs) of a batch: its sub-batches -----------------------------------------------------------------------
#define G16_MAX_PARTS 32
struct G16Part {
  size_t first, count;       // proofs [first, first + count) of the chunk: also the part's position in the workspace (proof units)
  int stream_slot;           // 0: the caller's stream, 1..3: auxiliary streams (concurrent parts); -1: not concurrent (the caller's stream)
};
struct G16ChunkPlan {
  int parts; size_t per;     // sub-batches and their nominal size (a multiple of 256)
  bool wide, concurrent, split_small;
  size_t max_launch;
  G16Part part[G16_MAX_PARTS];
};
// m: proofs of the chunk (<= G16_MAX_BATCH); key_inputs: len(vk.K) - 1; n_public: as passed by the caller; n_streams: BN254_STREAMS; single_stream: the device's
// sub-batch streams were measured NOT to overlap (they share a hardware queue): one sub-batch where one launch can hold the chunk
inline bool g16_plan_chunk(G16ChunkPlan& p, size_t m, size_t key_inputs, size_t n_public, int n_streams, bool single_stream) {
  p.wide = n_public == key_inputs && n_public > (size_t)G16_WIDE_MSM_MIN_INPUTS;
  p.max_launch = p.wide ? (size_t)G16_WIDE_MSM_MAX_PROOFS : (size_t)G16_MAX_LAUNCH;
  // Up to 65 536 proofs are one wavefront per SIMD at most: one sub-batch, and up to COOP12_MAX_PROOFS the cooperative kernels take the batch whole.  Above that,
  // n_streams sub-batches side by side (the tail of one sub-batch's kernel overlaps the head of the other's).  Keys with many inputs share ONE partial-sum
  // buffer between the launches of a batch, so their launches stay on the caller's stream and cover at most G16_WIDE_MSM_MAX_PROOFS proofs each.
  int parts = (!p.wide && n_streams > 1 && !single_stream && m > 65536) ? n_streams : 1;
  while ((m + parts - 1) / parts > p.max_launch) parts++;      // 32-bit workspace offsets per launch
  if (parts > G16_MAX_PARTS) return false;
  p.parts = parts;
  p.concurrent = !p.wide && n_streams > 1 && !single_stream && parts > 1;
  p.split_small = m <= (size_t)G16_SPLIT_MAX_PROOFS;
  p.per = g16_round256((m + parts - 1) / parts);
  int k = 0;
  for (int pi = 0; pi < parts; pi++) {
    const size_t lo = (size_t)pi * p.per, hi = lo + p.per < m ? lo + p.per : m;
    if (lo >= hi) break;
    p.part[k].first = lo; p.part[k].count = hi - lo; p.part[k].stream_slot = p.concurrent ? pi % 4 : -1;
    k++;
  }
  p.parts = k;
  return true;
}

// ---- BN254_FLAG_RLC: one workspace chunk, its launch parts and where their groups sit -------------------------------------------------------------------------
// A chunk of m proofs runs as `parts` launch parts; part pi forms rlc_plan(its proofs).groups groups.  Their status bytes sit in a region rounded up to 256
// (k_rlc_* grids are multiples of 256 lanes), one part's region after the other; for keys with more than RLC_MAX_PUBLIC inputs the group scalars and the groups'
// MSM scratch of the parts sit side by side, unrounded.  g16_plan_rlc_chunk is the ONE walk over the parts: rlc_ensure sizes from it, g16_enqueue_rlc addresses by
// it, bn254_dbg_g16_rlc_plan / _rlc_wide_plan / _rlc_groups show it.  g16_rlc_alloc(m) is what rlc_ensure allocates for the status bytes of a chunk of m proofs.
inline size_t g16_rlc_alloc(size_t m) { return g16_round256(m) + 1024; }
struct G16RlcPart {
  size_t first, count;       // proofs [first, first + count) of the chunk
  int log2_share;            // 2^log2_share proofs per lane of the Miller loop: at most the group, and only while the part keeps min_lanes lanes
  RlcPlan plan;
  size_t grp_off;            // its status region: the sum of round256(groups) of the parts before it
  size_t wide_off;           // its group scalars and MSM scratch (wide keys): the sum of the groups of the parts before it
};
struct G16RlcChunkPlan {
  int parts;
  size_t need;               // status bytes the parts address: against g16_rlc_alloc of the reservation
  size_t wide_groups;        // groups of all parts: what the wide buffers hold (g16_rlc_wide_alloc of it, rounded up to 256)
  G16RlcPart part[G16_MAX_PARTS];
};
// m: proofs of the chunk; n_streams: BN254_STREAMS; log2_group / log2_share_env: BN254_RLC_GROUP_LOG2 / BN254_RLC_SHARE_LOG2; min_lanes: bn254_set_rlc_params
inline bool g16_plan_rlc_chunk(G16RlcChunkPlan& p, size_t m, int n_streams, int log2_group, int log2_share_env, size_t min_lanes) {
  int parts = (n_streams > 1 && m >= (size_t)n_streams * 16384) ? n_streams : 1;
  while ((m + parts - 1) / parts > (size_t)G16_MAX_LAUNCH) parts++;
  if (parts > G16_MAX_PARTS) return false;
  const size_t per = g16_round256((m + parts - 1) / parts);
  p.parts = 0; p.need = 0; p.wide_groups = 0;
  for (int pi = 0; pi < parts; pi++) {
    const size_t lo = (size_t)pi * per, hi = lo + per < m ? lo + per : m;
    if (lo >= hi) break;
    G16RlcPart& q = p.part[p.parts++];
    q.first = lo; q.count = hi - lo;
    q.log2_share = log2_share_env < log2_group ? log2_share_env : log2_group;
    while (q.log2_share > 0 && (q.count >> q.log2_share) < (min_lanes < 1 ? 1 : min_lanes)) q.log2_share--;   // sharing needs enough lanes to fill the GPU
    q.plan = rlc_plan((uint32_t)q.count, log2_group, q.log2_share);
    q.grp_off = p.need; q.wide_off = p.wide_groups;
    p.need += g16_round256(q.plan.groups); p.wide_groups += q.plan.groups;
  }
  return true;
}

// ---- BN254_FLAG_RLC, keys with more than RLC_MAX_PUBLIC inputs: the group scalars and the groups' MSM scratch of one workspace chunk ------------------------
// bytes per group: its row of scalars (key_inputs x 32 B, big-endian like an input row), and for the tables of keys with more than 16 inputs (form 0: comb,
// 1: byte windows; 2: the 13-bit windows of up to 16 inputs need neither) the column digits (form 0) and the chunk sums of k_g16_msm_partial(_comb)
struct G16RlcWide { size_t rows_bytes, digit_bytes, part_bytes; };
inline G16RlcWide g16_rlc_wide_alloc(size_t groups, size_t key_inputs, int msm_form) {
  G16RlcWide a;
  const size_t chunks = (key_inputs + G16_WIDE_MSM_INPUTS_PER_LANE - 1) / G16_WIDE_MSM_INPUTS_PER_LANE;
  a.rows_bytes = groups * key_inputs * 32;
  a.digit_bytes = msm_form == 0 ? (size_t)G16_COMB_COLS * key_inputs * groups * sizeof(uint16_t) : 0;
  a.part_bytes = msm_form != 2 ? chunks * 27 * groups * sizeof(int32_t) : 0;
  return a;
}

// ---- BN254_FLAG_COMPRESSED_PROOFS: the decompression scratch of a (key, device) ------------------------------------------------------------------------------
// A compressed batch is decompressed and verified in chunks of at most G16_MAX_BATCH proofs (the chunk of the exact and the RLC paths): per proof one raw
// 256-byte record and one pre-status byte.  g16_cmp_alloc(n) is what a batch of n proofs needs (the pre bytes start at raw_bytes, a multiple of 256);
// ensure_scratch (bn254_capi_g16.hip) grows the scratch to it and the enqueue checks every chunk against it.
inline size_t g16_cmp_chunk(size_t n) { return n < (size_t)G16_MAX_BATCH ? n : (size_t)G16_MAX_BATCH; }
struct G16CmpAlloc { size_t proofs, raw_bytes, pre_bytes; };
inline G16CmpAlloc g16_cmp_alloc(size_t n) {
  G16CmpAlloc a;
  a.proofs = g16_round256(g16_cmp_chunk(n));
  a.raw_bytes = a.proofs * 256;
  a.pre_bytes = a.proofs;
  return a;
}

// ---- SP1 public inputs (bn254_verify.h, "SP1 proofs from their public values"): the row scratch of a (key, device) ----------------------------------------------
// An SP1 batch is hashed and verified in chunks of at most G16_MAX_BATCH proofs: per proof one 64-byte row vkey_hash | digest (the public inputs the raw
// pipeline reads, n_public = 2) and one pre-status byte.  g16_sp1_alloc(n) is what a batch of n proofs needs (the pre bytes start at row_bytes, a multiple of
// 256); ensure_scratch grows the scratch to it and the enqueue checks every chunk against it.
struct G16Sp1Alloc { size_t proofs, row_bytes, pre_bytes; };
inline G16Sp1Alloc g16_sp1_alloc(size_t n) {
  G16Sp1Alloc a;
  a.proofs = g16_round256(n < (size_t)G16_MAX_BATCH ? n : (size_t)G16_MAX_BATCH);
  a.row_bytes = a.proofs * 64;
  a.pre_bytes = a.proofs;
  return a;
}

}  // namespace bn254
