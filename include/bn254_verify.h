/*
 * bn254_verify.h -- C ABI of the MI355X-native batch BN254 verifier (libbn254_verify_amd.so).
 *
 * This is the drop-in boundary for the hot path of succinctlabs/snark-bn254-verifier.  The reference has no FFI of its
 * own; its only surface is the Rust API (paths relative to /root/reference):
 *     Groth16Verifier::verify(proof:&[u8], vk:&[u8], public_inputs:&[Fr]) -> Result<bool, Groth16Error>   verifier/src/lib.rs:44-49
 *     PlonkVerifier::verify(...)                                                                         verifier/src/lib.rs:69-74
 * and, below it, the `bn` crate calls that do all the work (groth16/verify.rs:70-77).  The entry points here are what a
 * thin Rust `extern "C"` wrapper binds to keep that surface and add `verify_batch(&[proof], &vk, &[[Fr]])`
 * (INTEGRATION.md shows the binding).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - All field elements cross the boundary as 32-byte big-endian integers, exactly as in gnark files.
 *   - Return value = infrastructure status (BN254_OK or a negative BN254_E_* code).  Per-proof outcomes are reported
 *     only through status bytes (BN254_REJECT ... below); nothing panics, unlike the reference's unwrap()s.
 *   - The caller owns every buffer it passes; the library owns the opaque prepared-vk handle.
 *   - A prepared vk is immutable and may be shared between threads.  The library keeps one workspace per (key, device): batches
 *     against the same key and device are serialised by the library itself (enqueue under a per-device lock, each batch waits
 *     on the previous batch's completion event before it touches the workspace), whatever streams the callers use.
 *     (PlonK keys hand out contexts instead and run calls side by side: see there.)  A handle must not be freed while a call that uses it is in flight
 *     on another thread; the free functions wait for the GPU work the handle has enqueued and release its device memory.
 *   - There is NO CPU fallback: every verify entry point runs the HIP kernels and fails with BN254_E_NO_DEVICE if
 *     no gfx950 device is usable.
 */
#ifndef BN254_VERIFY_H
#define BN254_VERIFY_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-proof status bytes (one per proof, written to status[]) ------------------------------------------------
 * Mapping to the reference's observable behaviour (verifier/src/...):                                            */
enum {
  BN254_REJECT = 0,              /* Ok(false): pairing equation does not hold           groth16/verify.rs:77          */
  BN254_ACCEPT = 1,              /* Ok(true)                                                                           */
  BN254_ERR_NOT_MEMBER = 2,      /* a proof coordinate >= p: Field(NotMember), a panic via unwrap   converter.rs:85-86,144-147, lib.rs:45 */
  BN254_ERR_NOT_ON_CURVE = 3,    /* Group(NotOnCurve)                                     converter.rs:87,152          */
  BN254_ERR_NOT_IN_SUBGROUP = 4, /* Group(NotInSubgroup), G2 point B only                 converter.rs:152             */
  BN254_ERR_INPUT_LEN = 5,       /* Err(PrepareInputsFailed): len(inputs)+1 != len(vk.K)  groth16/verify.rs:54-56      */
  BN254_ERR_MALFORMED = 6,       /* everything else the reference turns into a panic: short buffer, flag 0b00, no square root */
  BN254_ERR_OPENING_MISMATCH = 7,/* PlonK Error::OpeningPolyMismatch                      plonk/verify.rs:212-214      */
  BN254_ERR_PAIRING_FAILED = 8,  /* PlonK Error::PairingCheckFailed                       plonk/kzg.rs:185-187         */
  BN254_ERR_BSB22_MISMATCH = 9,  /* PlonK Error::Bsb22CommitmentMismatch                  plonk/verify.rs:52-54        */
  BN254_ERR_INVERSE = 10         /* PlonK Error::InverseNotFound                          plonk/verify.rs:106          */
};

/* ---- infrastructure return codes ----------------------------------------------------------------------------- */
enum {
  BN254_OK = 0,
  BN254_E_BAD_ARG = -1,
  BN254_E_NO_DEVICE = -2,   /* no usable HIP device / kernel image: the product never falls back to the CPU */
  BN254_E_HIP = -3,         /* a HIP runtime call failed; bn254_last_error() has the text */
  BN254_E_VK = -4,          /* the verifying key bytes do not load: whatever load_groth16_verifying_key_from_bytes / load_plonk_verifying_key_from_bytes turn into a panic
                               (short buffer, flag 0b00, no square root; groth16/converter.rs:28-89, plonk/converter.rs:18-119).  Status byte equivalent: BN254_ERR_MALFORMED.
                               A key that LOADS is never refused: no K points at all (every proof: loader error, else BN254_ERR_INPUT_LEN), G2 elements outside the r-torsion
                               (the loaders are "unchecked", converter.rs:113-133: computed on, as the reference does) */
  BN254_E_NOMEM = -5,
  BN254_E_SELFTEST = -6     /* the device failed its known-answer self-test (bn254_device_selftest below): nothing is launched on it, no status byte is written */
};

/* ---- verifying-key interpretation ---------------------------------------------------------
 * BN254_VK_REFERENCE reproduces the reference's actual input->output function: compressed G2 roots ordered by c0 only
 * (as the pinned `bn` does), beta negated on load (groth16/converter.rs:79) and the literal equation of
 * groth16/verify.rs:70-77.  BN254_VK_GNARK uses gnark-exact G2 decompression and gnark's equation
 * e(A,B) = e(alpha,beta) e(L,gamma) e(C,delta).  The two agree on every proof for verifying keys whose beta2, gamma2 have
 * y.c0 / y.c1 in different halves of [0,p) and delta2 in the same half (the SP1 key is presumably of this kind). */
enum { BN254_VK_REFERENCE = 0, BN254_VK_GNARK = 1 };

/* ---- per-call option flags of the batch entry points ------------------------------------------------------------
 * BN254_FLAG_STRICT_SCALARS  public inputs >= r are answered with BN254_ERR_NOT_MEMBER instead of being used modulo r.  The
 *     default (flag clear) is the reference's behaviour: bn::Fr::from_slice stores any 256-bit value and AffineG1 * Fr consumes it
 *     bit by bit, so x and x + r verify alike (examples/script/src/main.rs:204-213).  In the reference's
 *     typed API a range-checked Fr would fail at construction, before verify() is entered, so the strict error takes precedence
 *     over every proof error.
 * BN254_FLAG_RLC  random-linear-combination batch mode (the reference batches the same way inside KZG,
 *     plonk/kzg.rs:149-187): proofs are checked in groups with fresh random weights r_i (128 bits of entropy each),
 *         prod_i e(r_i A_i, B_i) * e(sum r_i L_i, gamma') * e(sum r_i C_i, delta') * e(-(sum r_i) alpha, beta') == 1,
 *     one variable-argument Miller loop per proof and one final exponentiation per group; proofs of a group that fails are
 *     re-verified by the exact path, so the status bytes are those of the exact path except with probability <= 2^-120 per batch
 *     (a false ACCEPT).  Loader errors (member / curve / subgroup) are always exact.  The weights come from ChaCha20 keyed by
 *     getrandom(2) per call.  The call synchronises the stream once (to learn which groups failed).
 *     The mode is a longer pipeline than the exact path and pays from about 200 000 proofs (2.0 x at 2^20): below that the flag is
 *     ignored (bn254_set_rlc_params, or BN254_RLC_MIN_BATCH in the environment when the library is loaded, moves the threshold; never below 64).
 *     Every key width is accepted.  Keys with more than 8 public inputs form the public-input sum once per group (group scalars sum_i r_i x_ij, then the key's own
 *     fixed-base tables), so the mode pays much earlier there: it is honoured from min(threshold above, 4096 + 6 000 000 / n_public) proofs -- about 10 000 at
 *     1024 inputs (4.2 x at 65 536), 27 500 at 256, the threshold above up to about 30 inputs -- the measured crossovers; BN254_RLC_WIDE_MIN_BATCH in the environment
 *     at load time replaces the formula by one value for all such keys.
 *     Adaptive: an RLC pass costs about half an exact pass and every proof of a failed group pays the exact pass on top, so per
 *     (key, device) the share of proofs that fell back is tracked, and while it is above 0.45 the flag is ignored (the exact path
 *     runs: same status bytes) except for one measuring RLC pass every 8 calls.  bn254_set_rlc_params(-1, 0, -1) (or
 *     BN254_RLC_ADAPTIVE=0 in the environment at load time) switches this off; bn254_groth16_rlc_state reports the tracked share (-1: no RLC pass yet) and the number of bypassed calls.
 * BN254_FLAG_COMPRESSED_PROOFS  (Groth16 batch entries only: bn254_groth16_verify_batch, _multi, which passes it to every shard, and _device; the PlonK
 *     entries refuse it, and bn254_groth16_verify takes no flags) every record starts with gnark's COMPRESSED proof, its default serialisation (WriteTo):
 *     A (32) | B (64: x.c1 | x.c0, the flag bits in the first byte) | C (32), so proof_stride >= 128; bytes past 128 are ignored.  The points are decompressed
 *     on the device (one proof per lane) and the raw pipeline runs on the result.  Definition: a compressed record has the status the raw path gives to the
 *     256-byte record bn254_g1_decompress(A, checked=0) | bn254_g2_decompress(B, BN254_VK_GNARK, checked=0) | bn254_g1_decompress(C, checked=0), except that
 *     if any of the three decompressions fails the status is BN254_ERR_MALFORMED (it takes precedence over BN254_ERR_INPUT_LEN and the strict-scalar error:
 *     the reference loads the proof before it prepares the inputs, lib.rs:45).  Consequences:
 *       - proof points always use gnark's lexicographic root order, whatever mode the key was prepared with (BN254_VK_REFERENCE's c0-only order is a quirk of
 *         the key loader);
 *       - decompression is unchecked: B's r-torsion is still tested by the pipeline, so BN254_ERR_NOT_IN_SUBGROUP stays possible;
 *       - BN254_ERR_NOT_MEMBER and BN254_ERR_NOT_ON_CURVE cannot occur (x >= p is silently reduced, a decoded point lies on its curve);
 *       - the codec's quirks carry over: flag 0b00 is MALFORMED; the G1 infinity flag is MALFORMED (3 is a non-residue); the G2 infinity flag gives the G2
 *         generator; an infinity flag with non-zero bits in the rest of its first 32 bytes is MALFORMED.
 *     Works with BN254_FLAG_RLC and BN254_FLAG_STRICT_SCALARS.  Device scratch: 257 bytes per proof of the largest compressed batch so far (at most 2^20 proofs:
 *     269 MB), allocated by the first compressed call that needs it -- bn254_groth16_reserve does not reserve it, so before capturing a compressed batch into a
 *     graph, run one compressed batch of at least that size on the (key, device). */
enum { BN254_FLAG_STRICT_SCALARS = 1u, BN254_FLAG_RLC = 2u, BN254_FLAG_COMPRESSED_PROOFS = 4u };

typedef struct bn254_g16_pvk bn254_g16_pvk;

/* Parse + decompress a gnark Groth16 verifying key ONCE (replaces the per-call load_groth16_verifying_key_from_bytes,
 * groth16/converter.rs:28-89, and the per-call pairing(alpha, beta), groth16/verify.rs:70): decompression, e(alpha,beta),
 * Miller-loop line tables for the two fixed G2 arguments.  Host work; no GPU needed: 3 ms for a 2-input key, 4 ms for 16 inputs, 14 ms for 1024.
 * The fixed-base tables for vk.K (13-bit windows, 13 MB per input; keys with more than 16 inputs: comb tables, 655 KB per input) are NOT built here: each device builds its
 * own copy from the key's K points on first use (bn254_groth16_reserve, or the first batch; csrc/bn254_k_comb.hip: 2 ms for 2 inputs, 17 ms for 1024), and the host keeps
 * 72 bytes per input (until round 5 the host built them: 9 ms for 2 inputs, 0.18 s for 16, 2.2 s for 1024 on 8 threads, and held the copy).  LIMIT a caller must still plan
 * for: 671 MB of DEVICE memory per 1024-input key and device (+ 226 MB of scratch during the construction); keep the handle, do not prepare per call.
 * BN254_TABLES_HOST=1 keeps the host construction. */
int bn254_groth16_vk_prepare(const uint8_t* vk, size_t vk_len, unsigned mode, bn254_g16_pvk** out);
void bn254_groth16_vk_free(bn254_g16_pvk* pvk);
/* number of public inputs the key expects (len(vk.K) - 1); SIZE_MAX for a key without K points: no input count satisfies groth16/verify.rs:54 */
size_t bn254_groth16_vk_num_public(const bn254_g16_pvk* pvk);

/* ---- Many keys prepared in one call ---------------------------------------------------------------------------------------------------------------
 * bn254_groth16_vk_prepare for n_keys keys at once, with the per-key work on `device` (csrc/bn254_k_vkprep.hip): the compressed points of all keys are decoded one
 * per lane, the two line tables of a key are walked projectively with ONE inversion per table (one lane per table), and e(alpha, beta) of all keys runs through the
 * one-pair pairing program.  What a caller with a list for bn254_groth16_verify_batch_keys does before its first batch.
 *   Definition of correctness.  For every i, key_status[i] is the return code of bn254_groth16_vk_prepare(vks[i], vk_lens[i], mode, &h): BN254_OK or BN254_E_VK.
 *   out[i] is NULL for a key that does not load; otherwise it is a handle indistinguishable from h: its host image (bn254_dbg_g16_pvk_image) is equal dword for dword
 *   and every entry point gives the same status bytes with it.  A key that fails does not disturb its neighbours.  The handles are independent of each other and of the
 *   call: each is freed with bn254_groth16_vk_free, in any order, and may share a key list with handles of the single-key function.
 *   Return value (infrastructure only): BN254_OK even when some keys fail.  BN254_E_BAD_ARG for a null pointer with n_keys > 0, a null vks[i] or mode > 1 -- reported
 *   before any device is touched.  n_keys == 0 returns BN254_OK and looks at nothing.  BN254_E_NO_DEVICE, BN254_E_HIP, BN254_E_NOMEM as elsewhere; on any negative
 *   return every out[i] is NULL and nothing is leaked.  There is no CPU fallback, as everywhere else in the library; with BN254_TABLES_HOST=1 in the environment
 *   (the host construction of every table) the entry loops over bn254_groth16_vk_prepare and needs no device.
 *   Behaviour.  Host-synchronous, on a stream of its own; safe from several host threads at once.  It touches no key's per-device state and builds no K-point tables:
 *   those stay lazy (bn254_groth16_reserve, the first batch), as for a handle of the single-key function.  The list is worked through in passes of at most 4096 keys
 *   and 2^18 compressed G1 points (a key with more points is a pass of its own), so the device scratch is bounded whatever n_keys is: 176 MB of line tables and
 *   pairing workspace at 4096 keys plus 104 bytes per G1 point, and as much pinned host memory for the way back; freed when the call returns.  Keys whose structure
 *   does not scan (a K count or a commitment-index count larger than the bytes that are there, a missing trailer) are refused on the host and never reach the device.
 *   Cost (one MI355X, profiles/r11_vk_prepare_batch.txt): a call costs 14 ms whatever the list holds up to a few hundred keys -- 9.2 ms of it the
 *   pairing program, a chain of small launches, 2.5 ms the line tables -- and grows from there: 1 key 14 ms, 256 keys 18 ms, 4096 keys 70 ms, 65 536 keys 0.74 s
 *   (17 / 11 us a key), 16 keys of 1024 inputs 15 ms.  The same keys through bn254_groth16_vk_prepare on that box, 1.6 ms a key: 4096 keys 6.5 s on one host thread and
 *   0.43 s on 16, 65 536 keys 104 s and 8.2 s.  CROSSOVER: against a loop on one host thread (a C or Rust caller) the batch entry wins from 16 two-input keys on (8
 *   keys: 14.5 ms against 12.7 ms), against a loop spread over 16 host threads from 256 keys on (64 keys: 15.7 ms against 11.1 ms).  Below that, prepare key by key. */
int bn254_groth16_vk_prepare_batch(const uint8_t* const* vks, const size_t* vk_lens, size_t n_keys, unsigned mode, int device, bn254_g16_pvk** out, int* key_status);

/* verify_batch on host buffers.  proofs: n records of proof_stride bytes (>= 256; bytes beyond 256 -- gnark's commitment
 * count / commitments / PoK -- are ignored exactly as in groth16/converter.rs:15-25; with BN254_FLAG_COMPRESSED_PROOFS: gnark's compressed
 * proof, >= 128 bytes, bytes beyond 128 ignored).  public_inputs: n * n_public * 32 bytes,
 * big-endian, NOT range-checked and used modulo r exactly like bn::Fr::from_slice + AffineG1 * Fr.
 * status: n bytes.  device: HIP device ordinal. */
int bn254_groth16_verify_batch(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride,
                               const uint8_t* public_inputs, size_t n_public, size_t n, uint8_t* status, int device, unsigned flags);
/* Same over several GPUs of the node: bit d of device_mask selects HIP device d.  The batch is cut into contiguous shards, one
 * host thread per device drives its shard through bn254_groth16_verify_batch, and the status bytes land in the caller's buffer
 * (the gather of SURVEY.md section 8(e) done by the host threads; a multi-process job gathers with RCCL instead, see bench.py). */
int bn254_groth16_verify_batch_multi(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride,
                                     const uint8_t* public_inputs, size_t n_public, size_t n, uint8_t* status,
                                     uint64_t device_mask, unsigned flags);
/* The shard plan bn254_groth16_verify_batch_multi follows (host arithmetic, no GPU): devices[k] = the k-th set bit of device_mask, its shard
 * the contiguous range [first[k], first[k] + count[k]) of the batch -- balanced, the first n % w shards one proof longer, the partition of
 * SURVEY.md section 8(e) (2^20 proofs over 8 GPUs = 131 072 each).  device_count = number of devices the caller has (a set bit at or
 * above it is BN254_E_BAD_ARG). */
int bn254_shard_plan(size_t n, uint64_t device_mask, int device_count, int devices[64], size_t first[64], size_t count[64], int* n_shards);

/* The gather of a multi-PROCESS job (one process per GPU, rank r verifying shard r of bn254_shard_plan(n, ranks 0..world-1)): ONE ncclAllGather of the
 * status bytes on hip_stream, every rank ends with the full n-byte vector in d_full (device memory).  nccl_comm: the caller's ncclComm_t (RCCL; the
 * library does not link RCCL: ncclAllGather is looked up in the process, then in librccl.so).  d_local: this rank's shard statuses (device memory).
 * d_scratch: world * ceil(n / world) bytes of device memory, needed only when n is not a multiple of world (ragged shards travel as padded blocks).
 * bench.py's ranks do the same through torch.distributed (snark-bn254-verifier_amd/sharding.py); this entry is for a Rust / C host. */
int bn254_status_all_gather(void* nccl_comm, int world, int rank, const void* d_local, size_t n, void* d_full, void* d_scratch, void* hip_stream);

/* Same, with proofs / public_inputs / status already resident in the memory of `device` (the bench path: inputs in
 * HBM when the timed region starts).  hip_stream is a hipStream_t (NULL = default stream); the call only enqueues
 * work and returns, so the caller synchronises the stream before reading status.  Use bn254_groth16_reserve() first to
 * keep the call free of allocations (graph capture). */
int bn254_groth16_verify_batch_device(const bn254_g16_pvk* pvk, const void* d_proofs, size_t proof_stride,
                                      const void* d_public_inputs, size_t n_public, size_t n, void* d_status,
                                      int device, void* hip_stream, unsigned flags);
/* pre-allocate the per-device workspace for batches of up to n proofs and upload the key's tables */
int bn254_groth16_reserve(const bn254_g16_pvk* pvk, size_t n, int device);

/* ---- Batches over many keys ---------------------------------------------------------------------------------------------------------------------------------
 * One call for proofs of many circuits.  pvks: a list of n_keys prepared keys (1 .. 65 536 entries; a handle may occur more than once; keys prepared with different
 * `mode`s may share a list).  Proof i is verified against pvks[key_index[i]] (key_index: n 32-bit unsigned little-endian words).  Its public inputs are the first
 * 32 * num_public(that key) bytes of row i of public_inputs; rows are input_stride bytes apart, and input_stride must be at least 32 * the largest num_public of the
 * list, else BN254_E_BAD_ARG (a list of keys without inputs may pass a null pointer and stride 0).
 *   DEFINITION OF CORRECTNESS: status[i] equals, byte for byte, what bn254_groth16_verify_batch(pvks[key_index[i]], proof_i, inputs_i, n_public =
 * bn254_groth16_vk_num_public(that key), 1, ..., flags without BN254_FLAG_RLC) writes; for a key without K points (num_public == SIZE_MAX), what that call writes
 * with n_public = 0.  n_keys == 1 gives the single-key bytes.
 *   key_index[i] >= n_keys: the host-buffer entry checks the whole vector first and returns BN254_E_BAD_ARG without touching status; the device entry cannot, writes
 * BN254_ERR_MALFORMED for that proof and verifies the others.
 *   Flags: BN254_FLAG_STRICT_SCALARS (the inputs checked are those of the proof's key) and BN254_FLAG_COMPRESSED_PROOFS work as in the single-key entries.
 * BN254_FLAG_RLC is accepted and IGNORED: by its contract the status bytes are those of the exact path, and that is the path a mixed batch takes (groups of the
 * random-linear-combination mode are per key; mixed-key groups do not exist yet).
 *   Limits of this revision, refused with BN254_E_BAD_ARG and a text in bn254_last_diagnostic(): a key with more than 16 public inputs in the list (such keys run
 * the wide multi-scalar-multiplication kernels, a different pipeline: one bn254_groth16_verify_batch call per key), and more than 65 536 entries.  A mixed batch has
 * no latency mode (the three Miller chains on three streams of the single-key entries) and no random-linear-combination groups.
 *   How it runs: in one of two forms, chosen from n alone (bn254_set_keys_params), with the same status bytes.  A SMALL batch -- up to keys_coop_max proofs -- takes
 * the DIRECT form: no grouping and no padding, the records are parsed in proof order and one cooperative kernel (twelve lanes per proof, five proofs per wavefront,
 * the key read per proof: the five proofs of a wavefront may belong to five keys) does the public-input sum, the Miller loop, the final exponentiation and the
 * verdict: two launches, as the small batches of the single-key entries.  A larger batch takes the GROUPED form: the proofs are grouped on the device so that
 * every wavefront (64 lanes) works for one key -- at most 63 idle lanes per key that has proofs -- and the one-proof-per-lane kernels run on those slots.  The
 * workspace of a reservation is that of n + min(n_keys, n) * 63 proofs whatever the form, since the knob may move between calls.  The host-buffer entry uploads
 * index, records and input rows first (through pinned memory) and then runs the same pipeline; it returns when the status bytes are back.
 *   Device state of a list: kept per (list of handles in order, device), the four most recently used lists, least recently used out first; bn254_groth16_vk_free of
 * a member drops every cached list that contains it (and a call with a list that names a freed key is undefined, as any use of a freed handle).  A list does NOT
 * build its members' own per-device tables (13 MB per K point): it keeps 38.5 KB of line tables per distinct key and byte-window tables of 652 800 bytes per K point
 * (a 2-input key: 1.3 MB; 4096 of them: 5.4 GB), built on the device at the list's first use.  bn254_groth16_reserve_keys returns BN254_E_NOMEM when they do not fit.
 *   bn254_groth16_reserve_keys does for a list what bn254_groth16_reserve does for a key: after it, a _device call with the same handles in the same order and up
 * to n proofs (raw records) allocates nothing and copies nothing from pageable memory.  The _device entry only enqueues on hip_stream (NULL = default stream). */
int bn254_groth16_verify_batch_keys(const bn254_g16_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride,
                                    const uint8_t* public_inputs, size_t input_stride, size_t n, uint8_t* status, int device, unsigned flags);
int bn254_groth16_verify_batch_keys_device(const bn254_g16_pvk* const* pvks, size_t n_keys, const void* d_key_index, const void* d_proofs, size_t proof_stride,
                                           const void* d_public_inputs, size_t input_stride, size_t n, void* d_status, int device, void* hip_stream, unsigned flags);
int bn254_groth16_reserve_keys(const bn254_g16_pvk* const* pvks, size_t n_keys, size_t n, int device);
/* Knob of the plan of a batch over many keys (process-wide, atomic; a negative value leaves it alone; initial value from BN254_KEYS_COOP_MAX, read once at load
 * time; default 30 720, the largest size at which the direct form was measured to gain at every key count: profiles/r10_multikey_small.txt): batches of up to
 * coop_max proofs take the direct form, larger ones the grouped form.  0: always the grouped form; values above 30 720 (the range of the cooperative kernels) are clamped; BN254_COOP=0 in the environment switches the direct form off whatever the knob says.  Same status bytes whatever the plan. */
void bn254_set_keys_params(long coop_max);

/* Groth16Verifier::verify (lib.rs:44-49) as one call: one proof, one status byte, vk given as bytes on every call like the
 * reference.  The prepared form of the last four keys (exact byte match, per mode) is kept, so only the first call with a key pays
 * its preparation (about 6.5 ms of an 8.5 ms call; 2 ms afterwards: profiles/r05_new_key_cost.txt); BN254_KEY_CACHE=0 in the environment switches the cache off, BN254_KEY_CACHE=N (1 .. 64) keeps the last N keys (default 4).
 * bn254_plonk_verify does the same.  Runs on the GPU (device 0).  The proof is the raw layout only: it takes no flags, so gnark's compressed proofs
 * (BN254_FLAG_COMPRESSED_PROOFS) go through the batch entries, with n = 1 if need be. */
int bn254_groth16_verify(const uint8_t* proof, size_t proof_len, const uint8_t* vk, size_t vk_len,
                         const uint8_t* public_inputs, size_t n_public, unsigned mode, uint8_t* status);

/* Raw gnark proof writer: A (64) | B (128: x.c1, x.c0, y.c1, y.c0) | C (64) | u32 0 (no commitments) | 64 zero bytes (commitment PoK):
 * the 324-byte form load_groth16_proof_from_bytes reads (groth16/converter.rs:14-26; SP1 fixtures carry exactly this). */
#define BN254_GROTH16_RAW_PROOF_LEN 324
int bn254_groth16_proof_write_raw(const uint8_t a[64], const uint8_t b[128], const uint8_t c[64], uint8_t out[BN254_GROTH16_RAW_PROOF_LEN]);

/* ---- PlonK (gnark / SP1 format), BASELINE configs[3] --------------------------------------------------------------
 * Replaces PlonkVerifier::verify (verifier/src/lib.rs:69-73) = load_plonk_proof_from_bytes (plonk/converter.rs:121-178) +
 * load_plonk_verifying_key_from_bytes (plonk/converter.rs:18-119, hoisted into vk_prepare) + verify_plonk
 * (plonk/verify.rs:46-317: Fiat-Shamir transcripts transcript.rs:15-108, BSB22 hash_to_field.rs:9-122, kzg::fold_proof and
 * kzg::batch_verify_multi_points plonk/kzg.rs:87-190).  Everything per proof runs on the GPU: the transcripts, the hash-to-field and the scalar-field
 * arithmetic as one-proof-per-lane kernels (csrc/bn254_k_plonk.hip, compiled from the same source as the host build of the stages that the library's
 * self-test checks them against), every group operation (24 G1 scalar multiplications and the two-pair pairing check per proof) as before.
 * Status bytes: BN254_ACCEPT or an error code; PlonK never returns BN254_REJECT (plonk/verify.rs:316).  Each proof occupies
 * proof_stride bytes (>= its length: 904 for the SP1 circuits); public inputs are n_public x 32 big-endian bytes per proof.
 * Threads: a prepared key may be used from several host threads at once.  Each call takes one of the key's eight per-device contexts (stream, device
 * buffers, pinned staging) per sub-batch of its plan (bn254_set_plonk_params) and a call that finds too few free waits; up to eight batches of 4096 are therefore in
 * flight on one key, which is how a verifier that always has requests pending should drive it: a single batch of that size is a chain of latency-bound
 * launches (1.06 M proofs/s), two in flight give 1.2-1.3 M proofs/s, four 1.4-1.6 M; calls of 65 536 proofs and more run at 2.5-3.1 M proofs/s. */
typedef struct bn254_plonk_pvk bn254_plonk_pvk;
int bn254_plonk_vk_prepare(const uint8_t* vk, size_t vk_len, bn254_plonk_pvk** out);
void bn254_plonk_vk_free(bn254_plonk_pvk* pvk);
size_t bn254_plonk_vk_num_public(const bn254_plonk_pvk* pvk);
int bn254_plonk_verify_batch(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                             size_t n_public, size_t n, uint8_t* status, int device);
/* The same with flags.  BN254_FLAG_RLC (round 4): the pairing checks of a pass are batched across proofs -- every proof's two points carry a random 128-bit
 * weight (drawn per call, folded into the scalars of the multi-scalar multiplication at no group cost), the weighted points of the 64 proofs of a wavefront are
 * added and ONE pairing check runs per group; the proofs of a group that fails are then checked one by one, so the status bytes are those of the exact path
 * except that a forged proof is accepted with probability ~2^-127 (weights are odd 128-bit values; the same kind of batching the reference applies to a proof's two openings, plonk/kzg.rs:149-187).
 * Honoured from 8192 proofs per pass (BN254_PLONK_RLC_MIN); below, the one remaining pairing is the same latency-bound launch and the flag changes nothing.
 * Any other flag bit is refused with BN254_E_BAD_ARG. */
int bn254_plonk_verify_batch_flags(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                                   size_t n_public, size_t n, uint8_t* status, int device, unsigned flags);
/* The same three entry shapes as Groth16 (north_star: one verify_batch surface for both verifiers):
 * _device  proofs, public inputs and status bytes resident in the memory of `device`.  Unlike the Groth16 entry this one is host-synchronous: it first waits for the work
 *          already enqueued on hip_stream (whatever still writes the inputs), runs the passes on the key's own context streams and returns when the status bytes are in
 *          d_status (a PlonK batch is several passes on several contexts driven by host threads, and BN254_FLAG_RLC has to read a counter back between two stages).
 * _multi   several GPUs of the node: the contiguous shards of bn254_shard_plan, one host thread per device through the host-buffer entry.
 * reserve  allocates NOW what a batch of up to n proofs needs on `device` (contexts of the plan, their buffers; proof_stride > 0: also the pinned staging of the host-buffer
 *          entry for records of that stride), so that the batch itself neither allocates nor frees.  Footprint per context, measured for the SP1 key shape (about 10 KB per proof of capacity plus
 *          1.8 KB per proof and variable MSM term): 0.16 GB for passes of up to 5040 proofs, 1.7 GB for 65 536, 3.5 GB for 131 072, 6.9 GB for 262 144; a batch above
 *          65 536 proofs uses up to eight contexts of its pass size (two for 262 144 proofs); beside them the window tables of the key's points, 131 MB for the reference's key
 *          (13 MB per point, built on the device at the key's first use).  bn254_plonk_footprint reports what a key holds on a device right now. */
int bn254_plonk_verify_batch_device(const bn254_plonk_pvk* pvk, const void* d_proofs, size_t proof_stride, const void* d_public_inputs, size_t n_public, size_t n,
                                    void* d_status, int device, void* hip_stream, unsigned flags);
int bn254_plonk_verify_batch_multi(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n,
                                   uint8_t* status, uint64_t device_mask, unsigned flags);
int bn254_plonk_reserve(const bn254_plonk_pvk* pvk, size_t n, size_t proof_stride, int device);
int bn254_plonk_footprint(const bn254_plonk_pvk* pvk, int device, size_t* bytes, int* contexts);
int bn254_plonk_verify(const uint8_t* proof, size_t proof_len, const uint8_t* vk, size_t vk_len, const uint8_t* public_inputs,
                       size_t n_public, uint8_t* status);
/* Knobs of the PlonK batch plan (process-wide, atomic; -1 leaves a knob alone; initial values from BN254_PLONK_PIECE / _WORKERS / _BIG_FROM / _BIG_PIECE, read once at
 * load time): below big_from proofs a batch is up to `workers` chains of passes of at most `piece` proofs side by side (latency-bound launches), from big_from on
 * few passes of up to big_piece <= 262144 proofs (throughput-bound launches).  big_from = 0 (the default) selects the plan measured on the MI355X: chains up to
 * ~9000 proofs, one pass up to ~20 000, two passes side by side up to ~40 000, one pass up to 65 536, passes of big_piece (default 131 072) on up to eight contexts beyond.
 * Same status bytes whatever the plan. */
void bn254_set_plonk_params(long piece, int workers, long big_from, long big_piece);
/* The pass size from which BN254_FLAG_RLC is honoured by the PlonK entries, on one key and over a key list (initial value: BN254_PLONK_RLC_MIN, default 8192: below,
 * the one remaining pairing is the same latency-bound launch as the per-proof checks).  Process-wide and atomic; never below 64 (a group is 64 proofs); a negative
 * value leaves it alone.  It changes no status byte. */
void bn254_set_plonk_rlc_params(long min_pass);
/* Durations (ms) of the first sub-batch of the bn254_plonk_verify_batch that finished last on `device`, from HIP events on the sub-batch's stream:
 *   [0] host: staging copy into pinned memory                                                           [1] k_plonk_stage1
 *   [2] k_g1_msm_rows of the linearised-polynomial digest   [3] its k_g1_sum_affine                   [4] k_plonk_stage2
 *   [5] k_g1_msm_rows of the KZG check (P0 and P1)          [6] their k_g1_sum_affine                 [7] the pairing check     [8] the sub-batch, host wall time
 * lanes: lanes (rows x items rounded up to 64) of the two k_g1_msm_rows launches. */
#define BN254_PLONK_NUM_TIMINGS 9
int bn254_plonk_last_timing(const bn254_plonk_pvk* pvk, int device, float ms[BN254_PLONK_NUM_TIMINGS], size_t lanes[2]);

/* ---- PlonK batches over many keys ---------------------------------------------------------------------------------------------------------------------------
 * One call for PlonK proofs of many circuits, the twin of bn254_groth16_verify_batch_keys.  pvks: a list of n_keys prepared keys (1 .. 256 entries; a handle may occur
 * more than once; the keys may differ in public-input count, domain size and KZG points).  Proof i is verified against pvks[key_index[i]] (key_index: n 32-bit
 * unsigned little-endian words).  Its public inputs are the first 32 * num_public(that key) bytes of row i of public_inputs; rows are input_stride bytes apart, bytes
 * behind a key's inputs are never read, and input_stride must be at least 32 * the largest num_public of the list, else BN254_E_BAD_ARG (a list of keys without
 * inputs may pass a null pointer and stride 0).  Records are proof_stride >= 808 + 96 * n_qcp bytes apart.
 *   DEFINITION OF CORRECTNESS: status[i] equals, byte for byte, what bn254_plonk_verify_batch_flags(pvks[key_index[i]], proof_i, inputs_i, n_public =
 * bn254_plonk_vk_num_public(that key), 1, ..., flags = 0) writes.  n_keys == 1 gives the single-key bytes.  Because the width of a row comes from the proof's key,
 * BN254_ERR_INPUT_LEN cannot occur.
 *   ALL ENTRIES OF A LIST MUST HAVE THE SAME NUMBER OF BSB22 COMMITMENTS: that number fixes the term counts and the multi-scalar-multiplication plans of a pass (one
 * list per commitment count).  A list that mixes counts, and one of more than 256 entries, is refused with BN254_E_BAD_ARG and a text in bn254_last_diagnostic().
 *   Argument errors (BN254_E_BAD_ARG, before any device is touched, status untouched): a null pointer with n > 0, an empty list, a null member, proof_stride below
 * 808 + 96 * n_qcp, input_stride below the widest key's row, any flag other than BN254_FLAG_RLC.  n == 0 returns BN254_OK and touches nothing.
 *   key_index[i] >= n_keys: the host-buffer entry checks the whole vector first, returns BN254_E_BAD_ARG, names the position in bn254_last_error() and leaves status
 * untouched; the device entry cannot, writes BN254_ERR_MALFORMED for that proof and verifies the others.
 *   BN254_FLAG_RLC is honoured from passes of bn254_set_plonk_rlc_params' min_pass slots on (default 8192, the single-key entry's threshold; smaller passes take
 * the exact path): the pairing checks of a pass are batched over its granules -- a granule's 64 slots hold proofs of one key, so it is a group as the 64 proofs of
 * a wavefront are on one key --, one cooperative check per group with the group's key, and only if a group fails the exact check runs, on the wavefronts of the
 * failed groups.  The status bytes are, as the flag's contract says, those of the exact path; a forged proof is accepted with probability ~ 2^-127, as on one key.
 *   How it runs: the proofs are grouped on the device so that every granule of 64 slots holds proofs of one key (at most 63 idle slots per key that has proofs), the
 * plan of the single-key entry (bn254_set_plonk_params) is made over slots with every cut on a granule boundary, and each pass gathers its records and input rows
 * into slot order, runs the stage, multi-scalar-multiplication and pairing kernels with the key read per granule, and scatters the status bytes back.  The per-proof
 * pairing check of a pass of up to bn254_set_plonk_keys_params' coop_max slots (default 40 960, the range of the cooperative kernel) runs in the cooperative form --
 * twelve lanes per slot, Miller loop, final exponentiation and verdict in one launch, the line tables of the slot's key fetched per lane --, larger passes in the
 * one-proof-per-lane (throughput) form; BN254_COOP=0 switches the cooperative form off.  Measured on one MI355X with the lane form for every pass
 * (profiles/r13_plonk_keys.txt; device-resident proofs of the SP1
 * key shape, n proofs spread evenly over K keys): one call beats one bn254_plonk_verify_batch_device call per key in every cell with K >= 4 -- n = 4096: 10.8 ms
 * against 13.3 ms (K = 4), 52.7 ms (16), 209 ms (64); n = 65 536: 20.5 / 20.9 / 21.2 ms against 41.2 / 55.5 / 213 ms; n = 262 144: 78.4 / 74.7 / 75.5 ms against
 * 82.8 / 166 / 222 ms -- and from 65 536 proofs on it takes 0.95 to 1.01 of the single-key entry's time on as many proofs of ONE key.  The cooperative form of a
 * pass and the flag over a list have NOT been measured yet (tools/bench_plonk_keys.py --lane --rlc takes the table; DESIGN.md section 9g says what is open): the
 * default of coop_max is the range of the cooperative kernel, as on one key, until that table says otherwise.
 *   Both entries are host-synchronous, like bn254_plonk_verify_batch_device; the _device entry first waits for hip_stream.  Calls on one list from several host threads
 * run side by side (the list owns eight pass contexts, leased as a key's are).
 *   Device state of a list: kept per (list of handles in order, device), the four most recently used lists; bn254_plonk_vk_free of a member drops every cached list
 * that contains it.  A list uses its members' OWN per-device tables: its first use makes every distinct member ready on the device (window tables of 13 MB per key
 * point, 131 MB for the SP1 key shape, and the key's self-test), after which the member is ready for single-key calls too.
 *   bn254_plonk_reserve_keys: after it, a call with the same handles in the same order, records of the same proof_stride and up to n proofs allocates nothing
 * (contexts for keys_slot_bound = n + min(n_keys, n) * 63 slots, the grouping buffers and the staging of the host-buffer entry for rows of 32 * the widest key);
 * BN254_E_NOMEM when the tables or the contexts do not fit.
 *   bn254_set_plonk_keys_params(coop_max): process-wide and atomic; passes of up to coop_max slots take the cooperative pairing form, 0: always the lane form; clamped
 * to 40 960; a negative value leaves the knob alone.  BN254_PLONK_KEYS_COOP_MAX, read when the library is loaded, gives the initial value.
 *   bn254_plonk_keys_state: counters of the cached (list, device) state since it was created -- out[0] passes that ran the joint check of BN254_FLAG_RLC, out[1] the
 * groups those passes checked (slots / 64 each), out[2] the groups that failed, out[3] passes whose per-proof pairing check ran in the cooperative form.
 * BN254_E_BAD_ARG for a null pointer or a list that is not cached (no batch or reservation yet, or evicted).
 *   Not in this revision: lists that mix commitment counts, the two-chain (latency) pairing form, a _multi entry, SP1 proofs from their public values over a list,
 * more than 256 entries, an adaptive bypass of the flag. */
int bn254_plonk_verify_batch_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride,
                                  const uint8_t* public_inputs, size_t input_stride, size_t n, uint8_t* status, int device, unsigned flags);
int bn254_plonk_verify_batch_keys_device(const bn254_plonk_pvk* const* pvks, size_t n_keys, const void* d_key_index, const void* d_proofs, size_t proof_stride,
                                         const void* d_public_inputs, size_t input_stride, size_t n, void* d_status, int device, void* hip_stream, unsigned flags);
int bn254_plonk_reserve_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, size_t n, size_t proof_stride, int device);
void bn254_set_plonk_keys_params(long coop_max);
int bn254_plonk_keys_state(const bn254_plonk_pvk* const* pvks, size_t n_keys, int device, uint64_t out[4]);

/* ---- gnark / SP1 formats, both directions (host only) ------------------------------------------------------------------
 * Point codecs of verifier/src/converter.rs:23-153.  compress: uncompressed big-endian coordinates (G1: x | y; G2: x.c1 | x.c0 |
 * y.c1 | y.c0) -> gnark compressed form (flag 0b10 / 0b11 = lexicographically smallest / largest y in the top two bits).
 * decompress: the inverse; `checked` selects compressed_x_to_g{1,2}_point (converter.rs:46,91: curve and, for G2, r-torsion
 * checks) over the unchecked variants (converter.rs:62,113) the key loaders use; mode = BN254_VK_REFERENCE / BN254_VK_GNARK
 * picks the reading of the G2 root order.  *status: BN254_ACCEPT, BN254_ERR_MALFORMED (flag 0b00, no square root),
 * BN254_ERR_NOT_ON_CURVE, BN254_ERR_NOT_IN_SUBGROUP.
 * bn254_sp1_fixture_parse: the SP1 v2.0.0 SP1ProofWithPublicValues files of examples/binaries/ (bincode) -> variant (2 PlonK,
 * 3 Groth16), raw gnark proof bytes, the two public inputs as 32-byte big-endian values, and the vkey hash: exactly what
 * examples/script/src/main.rs:115-138 feeds to the verifiers. */
int bn254_g1_compress(const uint8_t xy[64], uint8_t out[32]);
int bn254_g2_compress(const uint8_t xy[128], uint8_t out[64]);
int bn254_g1_decompress(const uint8_t in[32], uint8_t out[64], int checked, uint8_t* status);
int bn254_g2_decompress(const uint8_t in[64], uint8_t out[128], unsigned mode, int checked, uint8_t* status);
int bn254_sp1_fixture_parse(const uint8_t* buf, size_t len, int* variant, uint8_t* raw_proof, size_t raw_cap, size_t* raw_len,
                            uint8_t public_inputs[64], uint8_t vkey_hash[32]);

/* ---- SP1 proofs from their public values ---------------------------------------------------------------------------------------------------------------
 * An SP1 proof (SP1ProofWithPublicValues) is verified against the two circuit inputs vkey_hash | committed_values_digest (examples/script/src/main.rs:115-138),
 * and the caller holds the program's public values, not the digest:
 *     committed_values_digest = SHA-256(public_values) with the top three bits of byte 0 cleared.
 * bn254_sp1_public_values_digest computes it on the host.  The batch entries below compute it on the device, one proof per lane, and then run the unchanged
 * Groth16 or PlonK pipeline.  One SP1 circuit key serves every program of its SP1 version (the programs differ in vkey_hash, input 0), so one batch against
 * one prepared key may hold proofs of many programs.
 * Definition, for proof i of a batch of n:
 *   - its public values are the bytes [pv_offsets[i], pv_offsets[i+1]) of public_values; pv_offsets has n + 1 entries.  The offsets are absolute: a caller
 *     shards a batch by passing pv_offsets + first (and proofs, vkey hashes, status moved by `first` records) with the same public_values pointer;
 *   - its vkey hash is the 32 bytes at vkey_hashes + i * vkey_stride (big-endian, as bn254_sp1_fixture_parse writes it).  vkey_stride 0: one hash for the
 *     whole batch; any other stride must be at least 32;
 *   - its status is the status the matching RAW batch entry (bn254_groth16_verify_batch[_device], bn254_plonk_verify_batch_flags / _device) returns for the
 *     same proof record with n_public = 2 and the input row vkey_hash_i | digest_i, under the same flags: BN254_FLAG_STRICT_SCALARS (a vkey hash >= r is
 *     BN254_ERR_NOT_MEMBER; a digest is < 2^253 < r), BN254_FLAG_RLC and, for Groth16, BN254_FLAG_COMPRESSED_PROOFS.  A key whose width is not 2 therefore
 *     gives BN254_ERR_INPUT_LEN (or a loader status), as the raw entry does;
 *   - bad ranges.  Host-buffer entries read pv_offsets on the host: decreasing offsets are BN254_E_BAD_ARG before any device is touched.  The device entries
 *     take pv_bytes, the size of the buffer at d_public_values, and never read outside [0, pv_bytes): a proof with off[i] > off[i+1] or off[i+1] > pv_bytes
 *     gets BN254_ERR_MALFORMED, which overrides its pipeline status (the precedence of compressed records that do not decompress).
 * Every argument error (NULL pointers with n > 0, vkey_stride 1 .. 31, an unknown flag, STRICT or COMPRESSED on the PlonK entries, decreasing host offsets)
 * is BN254_E_BAD_ARG, reported before any device is touched; n = 0 returns BN254_OK.
 * The Groth16 entries hash into a per-(key, device) row scratch of 65 bytes per proof of the largest SP1 batch so far (chunks of at most 2^20 proofs: 68 MB),
 * allocated by the first SP1 call that needs it -- bn254_groth16_reserve does not reserve it, so before capturing an SP1 batch into a graph, run one SP1
 * batch of at least that size on the (key, device).  The host entry also stages the values, offsets and vkey hashes in per-(key, device) buffers.
 * bn254_sp1_groth16_verify_batch_device enqueues on hip_stream like bn254_groth16_verify_batch_device.  The PlonK entries keep the rows in memory of the
 * call (calls on one key run side by side), and bn254_sp1_plonk_verify_batch_device is host-synchronous like bn254_plonk_verify_batch_device. */
int bn254_sp1_public_values_digest(const uint8_t* public_values, size_t len, uint8_t out[32]);
int bn254_sp1_groth16_verify_batch(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* vkey_hashes, size_t vkey_stride,
                                   const uint8_t* public_values, const uint64_t* pv_offsets, size_t n, uint8_t* status, int device, unsigned flags);
int bn254_sp1_groth16_verify_batch_device(const bn254_g16_pvk* pvk, const void* d_proofs, size_t proof_stride, const void* d_vkey_hashes, size_t vkey_stride,
                                          const void* d_public_values, size_t pv_bytes, const uint64_t* d_pv_offsets, size_t n, void* d_status, int device,
                                          void* hip_stream, unsigned flags);
int bn254_sp1_plonk_verify_batch(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* vkey_hashes, size_t vkey_stride,
                                 const uint8_t* public_values, const uint64_t* pv_offsets, size_t n, uint8_t* status, int device, unsigned flags);
int bn254_sp1_plonk_verify_batch_device(const bn254_plonk_pvk* pvk, const void* d_proofs, size_t proof_stride, const void* d_vkey_hashes, size_t vkey_stride,
                                        const void* d_public_values, size_t pv_bytes, const uint64_t* d_pv_offsets, size_t n, void* d_status, int device,
                                        void* hip_stream, unsigned flags);

/* ---- Batch pairing-product checks over caller-supplied (G1, G2) pairs -----------------------------------------------------------------------------------------
 * The primitive both verifiers of the reference are built on, bn::pairing_batch(&[(G1, G2)]) (groth16/verify.rs:73-77, plonk/kzg.rs:175-187), without a key and
 * without a proof format: for a Groth16 key that is not a gnark file (snarkjs, arkworks, EVM calldata), a KZG opening of one's own, an fflonk or halo2-KZG tail,
 * or the EVM's ecPairing precompile (EIP-197) in bulk.  One item per lane on the device (new kernels, csrc/bn254_k_pairing.hip); up to eight pairs per item.
 *
 *   Definition.  Item i holds n_pairs records of BN254_PAIRING_PAIR_LEN = 192 bytes at pairs + i * item_stride: G1 x | y (64 bytes), then G2 x.c1 | x.c0 | y.c1 | y.c0
 *   (128 bytes), every coordinate 32 bytes big-endian -- gnark's order, which is also EIP-197's (the imaginary part first).  item_stride >= 192 * n_pairs; bytes past
 *   the records are ignored.  A point whose bytes are all zero is the identity; a pair with an identity on either side contributes 1 to the product, and its other
 *   point is still validated, as EIP-197 does.  status[i] is decided in two phases:
 *     phase 1  the first failure in record order (pair 0 G1, pair 0 G2, pair 1 G1, ...): a coordinate >= p gives BN254_ERR_NOT_MEMBER, otherwise a point off its
 *              curve gives BN254_ERR_NOT_ON_CURVE;
 *     phase 2  only if phase 1 found nothing: BN254_ERR_NOT_IN_SUBGROUP if any finite G2 point lies outside the r-torsion (G1 has cofactor 1: nothing to test);
 *     otherwise BN254_ACCEPT if prod_j e(P_j, Q_j) == 1, else BN254_REJECT.
 *   EIP-197 correspondence: the precompile's input is one item with item_stride = 192 * k; it returns 1 for BN254_ACCEPT, 0 for BN254_REJECT and fails (consumes all
 *   gas) for the three error codes.  More than eight pairs per call are not taken in this revision.
 *
 *   bn254_pairing_batch writes, instead of the verdict, the final-exponentiated product prod_j e(P_j, Q_j) of item i to out_gt + 384 * i in format 0 of the probes
 *   (12 x 32 bytes big-endian, tower order, as bn254_dbg_pairing), and status[i] = BN254_ACCEPT where that value is valid; otherwise status[i] is the error of phase 1
 *   or 2 and the item's 384 bytes are unspecified.
 *
 *   Argument errors (BN254_E_BAD_ARG before any device is touched, status untouched): a null pointer with n > 0, n_pairs 0 or above BN254_PAIRING_MAX_PAIRS, an
 *   item_stride below 192 * n_pairs.  n == 0 returns BN254_OK.  There is no CPU fallback (BN254_E_NO_DEVICE); the first use of a device runs the device self-test
 *   (below) as every other entry that makes a device ready, bn254_pairing_reserve included.
 *
 *   One workspace per device (4680 bytes per item, for at most 2^18 items: a larger batch runs as several launches), shared by all calls: calls on a device are
 *   serialised like the calls on a (key, device) of the Groth16 entries -- the enqueue under a lock, after a wait on the GPU for the previous call's completion --
 *   and are safe from several host threads.  bn254_pairing_check_batch_device only enqueues on hip_stream (the caller synchronises it), like
 *   bn254_groth16_verify_batch_device; once bn254_pairing_reserve(n', device) with n' >= min(n, 2^18) has returned it allocates nothing.  The host-buffer entries
 *   stage the records through pinned memory in passes (at most 2^18 items and 48 MB of records each) and return with the status bytes.
 *
 *   Two forms of a launch, with the same status and GT bytes.  The lane form (one item per lane) fills the GPU from about 16 384 items; below that its time is one
 *   wavefront's instruction stream whatever the size.  A launch of up to coop_max items therefore takes the COOPERATIVE form: the same loader, then one kernel with
 *   twelve lanes per item (csrc/bn254_coop12.hip, k_coop12_miller_pairs) that runs the Miller loop of every pair, the r-torsion tests and the final exponentiation.
 *   bn254_set_pairing_params(coop_max): process-wide and atomic; 0: always the lane form; clamped to 30 720, the cooperative kernels' range; negative: unchanged.
 *   Default 16 384, the largest measured size at which it is not slower than the lane form at any pair count (4096 items of 1 / 8 pairs: 1.7 / 6.6 ms against
 *   8.9 / 31.5 ms).  The environment variable BN254_PAIRING_COOP_MAX gives the initial value, BN254_COOP=0 switches the cooperative form off.  A launch takes one
 *   form whole.  bn254_pairing_params reads the knob back (out[0] = coop_max); bn254_pairing_state counts the launches enqueued so far by this process: out[0] in the
 *   cooperative form, out[1] in the lane form. */
#define BN254_PAIRING_MAX_PAIRS 8
#define BN254_PAIRING_PAIR_LEN 192   /* G1 x | y (64)  then  G2 x.c1 | x.c0 | y.c1 | y.c0 (128): gnark's order, which is also EIP-197's */
int bn254_pairing_check_batch(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* status, int device);
int bn254_pairing_check_batch_device(const void* d_pairs, size_t item_stride, size_t n_pairs, size_t n, void* d_status, int device, void* hip_stream);
int bn254_pairing_batch(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* out_gt /* n x 384 */, uint8_t* status, int device);
int bn254_pairing_reserve(size_t n, int device);
void bn254_set_pairing_params(long coop_max);
int bn254_pairing_params(long out[1]);
int bn254_pairing_state(uint64_t out[2]);

/* ---- Pairing batches with shared, prepared G2 points ------------------------------------------------------------------------------------------------------------
 * In the uses named above most G2 arguments are the same point in every item: a restated Groth16 proof has one variable G2 (B) and three of the key (beta, gamma,
 * delta); a KZG check has [1]_2 and [tau]_2 and no other.  A caller says so per POSITION of the item: bit j of shared_mask (j < n_pairs) means "the G2 point of
 * position j is this one, for every item" (arkworks' G2Prepared, gnark's precomputed lines).
 *
 *   bn254_g2_prepare (host work, no device) turns the 128 bytes x.c1 | x.c0 | y.c1 | y.c0 of a G2 point -- the G2 half of a pair record -- into a PREPARED RECORD of
 *   BN254_G2_PREPARED_LEN bytes: a header of four dwords (a magic word, the layout version, flags with bit 0 = identity, a reserved word), the affine point as the
 *   four field elements of the workspace layout, and the 88 affine lines of the optimal-ate loop in the encoding of the key tables (54 dwords each).  *status:
 *   BN254_ACCEPT, out written; or BN254_ERR_NOT_MEMBER, BN254_ERR_NOT_ON_CURVE, BN254_ERR_NOT_IN_SUBGROUP -- the checks of phase 1 and phase 2 of the definition
 *   above, in that order -- and out untouched.  The return code is BN254_OK in all four cases (as bn254_g2_decompress); a null pointer returns BN254_E_BAD_ARG.
 *   All-zero bytes are the identity: accepted, and flagged in the record.  The record is plain data: the caller owns it, may keep it beside its key, and copies it to
 *   the device itself (no handle, no lifetime, no per-device state).  A record is valid only for the layout version that wrote it: keep the 128 bytes, not the record,
 *   across versions of the library.
 *
 *   The entries.  prepared holds popcount(shared_mask) records, in ascending position order.  The item is PACKED: a shared position occupies BN254_PAIRING_G1_LEN = 64
 *   bytes (G1 x | y), a variable position 192 bytes as above, positions in order; item_stride >= the sum.  d_prepared must be 4-byte aligned (the lines are fetched
 *   by dword loads at wavefront-uniform addresses).
 *   Definition: status[i] and the GT value are those bn254_pairing_check_batch / bn254_pairing_batch give the EXPANDED item, in which every shared position carries
 *   the 128 bytes its record was prepared from.  So: phase 1 runs in record order over what the record holds (for a shared position the G1 point alone); the r-torsion
 *   test applies to the variable positions (with every position shared BN254_ERR_NOT_IN_SUBGROUP cannot occur); a shared identity makes its pair contribute 1 while its
 *   G1 point is still validated; the GT bytes are identical (the affine line of a table differs from the projective one by a factor in Fp2, which the final
 *   exponentiation removes -- what the Groth16 path has relied on since its first revision).
 *   Argument errors (BN254_E_BAD_ARG before any device is touched, status untouched): those of the entries above, a bit of shared_mask at or above n_pairs, prepared
 *   null with a non-zero mask, an item_stride below the packed size, and -- in the host entries, which can read it -- a record whose magic word or version is wrong.
 *   bn254_pairing_check_batch_shared_device cannot read the record on the host: its loader kernel reads the header words, and on a mismatch every item of the call
 *   ends as BN254_ERR_MALFORMED and no table is read.  shared_mask == 0 is the entry above: same kernels, same bytes.
 *   Workspace, reservation (bn254_pairing_reserve), locking and passes are those of the entries above; a host call stages the prepared records with every pass's items
 *   (so a pass holds 48 MB less popcount * 19 168 bytes of items).  Launches count in bn254_pairing_state by their form as well.
 *   Kernels: the lane form reads the packed item (k_pairing_load_shared) and runs k_miller_run_mix -- per step the G2 step and line of every variable position, then one
 *   table-driven line product per shared position, no G2 arithmetic, no r-torsion test and no G2 bytes for those.  A launch of up to coop_max items takes the
 *   cooperative form after the same loader; that form gains nothing from the tables (the shared point is in the workspace as if it had come from the item). */
#define BN254_G2_PREPARED_LEN 19168  /* (4 + 4 * 9 + 88 * 54) * 4; a static_assert in csrc/bn254_capi_pairing.hip holds it to the structures */
#define BN254_PAIRING_G1_LEN 64      /* a shared position of a packed item: G1 x | y */
int bn254_g2_prepare(const uint8_t g2[128], uint8_t out[BN254_G2_PREPARED_LEN], uint8_t* status);
int bn254_pairing_check_batch_shared(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared,
                                     size_t n, uint8_t* status, int device);
int bn254_pairing_check_batch_shared_device(const void* d_items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const void* d_prepared,
                                            size_t n, void* d_status, int device, void* hip_stream);
int bn254_pairing_batch_shared(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared,
                               size_t n, uint8_t* out_gt /* n x 384 */, uint8_t* status, int device);

/* ---- BN254_FLAG_RLC for the pairing-product check ------------------------------------------------------------------------------------------------------------------
 * bn254_pairing_check_batch_flags[_device] are bn254_pairing_check_batch_shared[_device] with a flags word: items, packing, shared_mask, prepared, argument errors,
 * workspace, lock and reservation are theirs; shared_mask == 0 with prepared == NULL is the all-variable item.  flags may hold BN254_FLAG_RLC only (anything else is
 * BN254_E_BAD_ARG); with flags == 0 the entry runs exactly the launches the shared entry runs.  bn254_pairing_batch* (GT values out) takes no flag.
 *
 *   BN254_FLAG_RLC: every item that passes phase 1 draws a fresh odd 128-bit weight r_i -- ChaCha20 block i of a key drawn with getrandom(2) once per call, the launch
 *   number in a nonce word -- and every finite G1 point of it is replaced by r_i P_ij (G1 has cofactor 1, so no identity flag changes).  The Miller loop then runs per
 *   item over the VARIABLE positions alone, without a final exponentiation; the r-torsion test of every variable G2 point decides at its end exactly as in the exact
 *   entry (BN254_ERR_NOT_IN_SUBGROUP).  Behind it the 64 consecutive items of a wavefront form a group: per shared position the sum of the pending items' weighted
 *   points, and the product of their Miller values; ONE table-driven Miller loop over the shared positions, one product and ONE final exponentiation decide the
 *   group.  A group that passes accepts its pending items; the items of a failed group go through the exact check on their weighted points (r_i is invertible mod r and
 *   GT has prime order r, so the verdict is that of the unweighted item).
 *   Contract: the status bytes are those of the exact entry, except that a false BN254_ACCEPT has probability about 2^-127 per item (a forged item passes only if a
 *   non-trivial relation in the random r_i holds; the reasoning of bn254_kzg_verify_batch).  The flag is honoured for a launch of rlc_min items or more
 *   (bn254_set_pairing_rlc_params: process-wide, atomic, a negative value leaves it alone, never below 64; initial value BN254_PAIRING_RLC_MIN; read back by
 *   bn254_pairing_rlc_params) whose items have NO variable position (every position shared); any other launch is the exact launch and counts in out[3].  With the flag honoured BOTH entries synchronise ONCE per launch, to
 *   learn which groups failed; a launch that does not honour it is the exact launch, and then bn254_pairing_check_batch_flags_device only enqueues on hip_stream and,
 *   after bn254_pairing_reserve, allocates nothing.  The weighted form grows a group workspace and status bytes of its own under the device's lock.
 *   bn254_pairing_rlc_state: out[0] launches that ran the joint check, out[1] the groups they checked, out[2] the groups that failed, out[3] launches of these
 *   entries on the exact path (flags == 0 goes through the shared entry and counts nowhere here).
 *   out[1] counts the groups of every joint launch, ceil(m / 64), whether or not a group holds a pending item; out[2] those whose check failed.
 *   Measured on one MI355X (profiles/r20_pairing_rlc.txt, tools/bench_pairing.py --rlc; device-resident all-valid items, flag | exact alternating, median of 5):
 *   (2, 0b11) 4.43 | 2.33 ms at 4096 items, 4.44 | 8.89 at 16 384, 4.71 | 9.28 at 65 536; (8, 0xff) 15.1 | 6.5, 15.2 | 24.5, 15.8 | 17.4; (4, 0b1110) 15.5 | 3.8, 15.5 | 14.2,
 *   16.6 | 14.9; (1, 0) 6.7 | 1.6, 6.7 | 6.1, 7.3 | 10.1; (4, 0) 19.7 | 3.8, 19.8 | 14.3, 21.4 | 20.7; (8, 0) 36.9 | 6.6, 37.2 | 24.5, 39.9 | 34.6 -- spreads below 0.3 ms.
 *   The 262 144-item rows the rule was also to be read from could not be produced (every attempt lost its GPU machine before the command ran): K = 0 and the
 *   default rest on three sizes, with the losing ratios still falling with n, and are PROVISIONAL until `tools/bench_pairing.py --rlc ... --sizes 262144` has been run.
 *   The default of rlc_min is 16 384, the smallest measured size at which the flag wins at (2, 0b11).  This DEPARTS from the rule the entry was specified with, a win at
 *   (2, 0b11) AND at (4, 0b1110): (4, 0b1110) wins at no size up to 65 536, so that rule gives no threshold and (2, 0b11) alone sets it ((8, 0xff) agrees).  K = 0: a
 *   shape with more than 0 variable positions is not honoured, because (4, 0b1110), (4, 0) and (8, 0) lose at 4096, 16 384 and 65 536 (those lines of the profile), and
 *   a rule by the count of variable positions cannot honour (1, 0), which wins at 65 536, without honouring (4, 0b1110).  K = 0 comes from THIS implementation, not
 *   from the method: the weight step is a plain 128-step double-and-always-add per G1 point and lane with one inversion per point, run for identity positions too -- one
 *   dependent chain per SIMD, so the weighted time hardly moves with n up to 65 536 and grows with the points per item (4.4 ms for two, 15 for four).  A windowed
 *   multiplication with a shared inversion would move every line; until then the joint check of shapes with a variable position (k_miller_run_sub,
 *   k_pairing_rlc_group_prod) is reachable through the probes alone.  With one invalid item in every group of 64 (the worst case of the fallback) 65 536 items of
 *   (2, 0b11) take 13.9 ms against 9.2 exact, of (8, 0xff) 32.9 against 17.1.  Not measured: 262 144 items (the runs could not be made: see DESIGN.md section 9j.2), the host entry.
 *   Kernels: the loader of the exact entry, k_pairing_rlc_weigh, k_miller_run_sub (k_miller_run_var when no position is shared) in the lane form at every size,
 *   k_pairing_rlc_group_sums, k_pairing_rlc_group_prod, then on the groups the launches of the exact entry in the form bn254_set_pairing_params gives their count,
 *   k_plonk_group_scatter, and after the synchronisation the exact launch behind its loader for the items of failed groups. */
int bn254_pairing_check_batch_flags(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared,
                                    size_t n, uint8_t* status, int device, unsigned flags);
int bn254_pairing_check_batch_flags_device(const void* d_items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const void* d_prepared,
                                           size_t n, void* d_status, int device, void* hip_stream, unsigned flags);
void bn254_set_pairing_rlc_params(long rlc_min);
int bn254_pairing_rlc_params(long out[1]);
int bn254_pairing_rlc_state(uint64_t out[4]);   /* [0] launches that ran the joint check, [1] groups they checked, [2] groups that failed, [3] launches on the exact path */

/* ---- Batch verification of KZG openings ---------------------------------------------------------------------------------------------------------------------------
 * The reference's plonk/kzg.rs::batch_verify_multi_points (lines 128-190) for openings a caller holds (a KZG opening of one's own, an fflonk or halo2-KZG tail): the
 * G1 fold runs on the device, the pairing check is the shared-G2 batch above.
 *
 *   An OPENING is BN254_KZG_OPENING_LEN = 192 bytes: the commitment C x | y, the quotient H x | y, the point z, the claimed value y -- 32-byte big-endian each.
 *   A KEY is BN254_KZG_KEY_LEN bytes of plain data (no handle, no lifetime, no per-device state -- like a prepared G2 record, and valid for the layout version that
 *   wrote it): 16 bytes (a magic word, the layout version, flags with bit 0 = g1 is the identity, a reserved word), g1 as the two field elements of the workspace
 *   layout (72 bytes), and the prepared records of g2 and tau_g2, byte for byte what bn254_g2_prepare writes.
 *
 *   bn254_kzg_key_prepare (host work, no device): *status is BN254_ACCEPT and out written, or the first failure over g1, g2, tau_g2 -- BN254_ERR_NOT_MEMBER,
 *   BN254_ERR_NOT_ON_CURVE and, for the G2 points, BN254_ERR_NOT_IN_SUBGROUP -- and out untouched.  The return code is BN254_OK in all of these cases; a null pointer
 *   returns BN254_E_BAD_ARG.  All-zero bytes are the identity: accepted and flagged.
 *
 *   Definition of status[i] (flags without BN254_FLAG_RLC), in this order:
 *     1. With BN254_FLAG_STRICT_SCALARS a z or y >= r is BN254_ERR_NOT_MEMBER; without it the scalars are used modulo r, the library's convention everywhere.
 *     2. The points in record order, C then H: a coordinate >= p is BN254_ERR_NOT_MEMBER, a point off the curve BN254_ERR_NOT_ON_CURVE; all-zero is the identity.
 *     3. BN254_ACCEPT if e(C - y g1 + z H, g2) e(-H, tau_g2) == 1, else BN254_REJECT.
 *   Equivalently: what bn254_pairing_check_batch_shared gives the two-pair item (F_i, -H_i), F_i = C_i - y_i g1 + z_i H_i, with mask 0b11 and the key's two records.
 *   A pair with an identity on either side contributes 1; BN254_ERR_NOT_IN_SUBGROUP cannot occur.
 *   Argument errors (BN254_E_BAD_ARG before any device is touched, status untouched): a null pointer with n > 0, a stride below 192, any flag other than
 *   BN254_FLAG_STRICT_SCALARS and BN254_FLAG_RLC, a d_key that is not 4-byte aligned and -- in the host entry -- a key whose magic word or version is wrong.  The device
 *   entry cannot read the key on the host: its loader kernel reads the header words, and on a mismatch every opening ends BN254_ERR_MALFORMED and no table is read.
 *   n == 0 returns BN254_OK.
 *
 *   BN254_FLAG_RLC (the reference's batching, across openings): every opening gets a fresh odd 128-bit weight r_i -- ChaCha20, expanded on the device from a key drawn
 *   with getrandom(2) once per call -- folded into its scalars: F'_i = r_i C_i + (r_i z_i) H_i - (r_i y_i) g1, H'_i = -r_i H_i.  The weighted points of the 64 openings
 *   of a wavefront are summed (decided openings and identities drop out) and one two-pair check runs per group; a group that passes accepts its pending openings, the
 *   openings of a failed group go through the per-opening check on their weighted points (r_i is invertible mod r: the verdict is that of the unweighted points).
 *   Contract: the status bytes are those of the exact path, except that a false ACCEPT has probability about 2^-127.  The flag is honoured from rlc_min openings per
 *   launch on (bn254_set_kzg_params: process-wide, atomic, a negative value leaves it alone, never below 64; initial value BN254_KZG_RLC_MIN, default 65 536; read
 *   back by bn254_kzg_params).  With the flag honoured BOTH entries synchronise once per launch to learn which groups failed, as the Groth16 flag does.  Without it
 *   bn254_kzg_verify_batch_device only enqueues on hip_stream, and after bn254_kzg_reserve(n', device) with n' >= min(n, 2^18) it allocates nothing.
 *   bn254_kzg_state: out[0] launches that ran the joint check, out[1] the groups they checked, out[2] the groups that failed, out[3] launches on the exact path.
 *
 *   Measured on one MI355X (profiles/r17_kzg_batch.txt, tools/bench_kzg.py; device-resident valid openings, exact | BN254_FLAG_RLC honoured | the pairing alone on
 *   the same openings with F_i precomputed, median of 5 alternating calls): 4096 openings 2.98 | 2.98 | 2.27 ms, 65 536 openings 10.73 | 5.16 | 9.32 ms, 262 144
 *   openings 35.99 | 13.74 | 30.88 ms.  So the exact entry costs 1.15 .. 1.31 of its pairing, and the weighted call ties at 4096 and takes 0.48 and 0.38 of the exact
 *   time at the two larger sizes: the default of rlc_min is 65 536, the smallest measured size where it wins by more than the spread.
 *   Workspace and locking: the per-device workspace, lock and completion event of the pairing batch (a KZG call and a pairing call on one device serialise), plus the
 *   term records, rows and window-table scratch of the G1 walk (about 4.5 KB per opening of the largest launch; the weighted form twice that and the groups).  A launch
 *   holds at most 2^18 openings; the host entry stages the key and the openings in passes through pinned memory.  The first use of a device runs the self-test.
 *   Kernels: k_kzg_load (checks, scalars mod r, the weight, glv_decompose, term records), k_g1_msm_rows / k_g1_sum_affine (the G1 walk; g1 is walked as a variable
 *   term, a plain-data key has no window table), k_kzg_ident, then the launches of the pairing batch behind its load step; weighted: k_plonk_group_sums /
 *   k_plonk_group_scatter around the groups' check. */
#define BN254_KZG_OPENING_LEN 192    /* commitment x|y (64) | quotient H x|y (64) | point z (32) | claimed value y (32), big-endian */
#define BN254_KZG_KEY_LEN 38424      /* 16 (magic, layout version, flags: bit 0 = g1 is the identity, reserved) + 72 (g1 affine, workspace digits) + 2 * BN254_G2_PREPARED_LEN; a static_assert in csrc/bn254_capi_kzg.hip holds it to the structures */
int bn254_kzg_key_prepare(const uint8_t g1[64], const uint8_t g2[128], const uint8_t tau_g2[128], uint8_t out[BN254_KZG_KEY_LEN], uint8_t* status);
int bn254_kzg_verify_batch(const uint8_t* key, const uint8_t* openings, size_t stride, size_t n, uint8_t* status, int device, unsigned flags);
int bn254_kzg_verify_batch_device(const void* d_key, const void* d_openings, size_t stride, size_t n, void* d_status, int device, void* hip_stream, unsigned flags);
int bn254_kzg_reserve(size_t n, int device);
void bn254_set_kzg_params(long rlc_min);
int bn254_kzg_params(long out[1]);
int bn254_kzg_state(uint64_t out[4]);   /* [0] launches that ran the joint check, [1] groups they checked, [2] groups that failed, [3] launches on the exact path */

/* ---- Batch verification of KZG batch-opening proofs (k commitments at one point, one quotient) ----------------------------------------------------------------------
 * The other half of the reference's KZG layer, plonk/kzg.rs::fold_proof (lines 46-126; gnark's BatchOpeningProof / BatchVerifySinglePoint), for proofs a caller holds:
 * several committed columns opened at one point -- a PlonK variant of one's own, a lookup argument.  The fold runs on the device; the key is the KZG key of above.
 *
 *   A RECORD is BN254_KZG_FOLD_LEN(k, data_len) = 96 + 96 k + data_len bytes: the digests D_0 .. D_{k-1} (x | y, 64 bytes each), the quotient H (64), the point z (32),
 *   the claimed values y_0 .. y_{k-1} (32 each), then data_len bytes of caller data that only the transcript reads.  Field values are 32-byte big-endian, an all-zero
 *   point is the identity.  k = n_digests and data_len are the same for every record of a call: 1 <= k <= BN254_KZG_FOLD_MAX_DIGESTS, data_len <=
 *   BN254_KZG_FOLD_MAX_DATA, stride >= the record length -- anything else is BN254_E_BAD_ARG before any device is touched, as are the argument errors of
 *   bn254_kzg_verify_batch.  With k = 1 and data_len = 0 a record is an opening, and the status bytes are those of bn254_kzg_verify_batch.  With k = 1 the
 *   fold does not depend on gamma (only gamma^0 = 1 enters it): the entries then run the opening's loader kernel, hash nothing and do not read the data bytes at all.
 *   A device or pinned allocation that fails for lack of memory is BN254_E_NOMEM in these three entries.
 *   BN254_KZG_FOLD_MAX_DIGESTS is the largest k for which both forms of the G1 walk plan whatever the batch size: the weighted form has k + 3 variable terms, a
 *   small launch walks each in two rows, and a launch has 32 rows (csrc/bn254_msm.h; a static_assert in csrc/bn254_kzg.h and tests/test_kzg_fold_cpu.py hold it there).
 *
 *   status[i]:  gamma = SHA-256("gamma" | be32(z mod r) | D_0 .. D_{k-1} as they stand in the record | be32(y_0 mod r) .. be32(y_{k-1} mod r) | data) read big-endian
 *   and reduced mod r (transcript.rs:68-107 with one challenge and no predecessor, kzg.rs:46-72);  D = sum gamma^i D_i,  y^ = sum gamma^i y_i;  BN254_ACCEPT iff
 *   e(D - y^ g1 + z H, g2) e(-H, tau_g2) == 1, else BN254_REJECT.  Loader errors in the order of bn254_kzg_verify_batch: with BN254_FLAG_STRICT_SCALARS any of z, y_i
 *   >= r is BN254_ERR_NOT_MEMBER first; then the points in record order, the digests before H, inside a point a coordinate >= p (NOT_MEMBER) before the curve equation
 *   (NOT_ON_CURVE); a malformed key makes every record BN254_ERR_MALFORMED.
 *
 *   BN254_FLAG_RLC has the meaning it has for openings -- one odd 128-bit weight per record folded into all its scalars, the weighted points of the 64 records of a
 *   wavefront summed, one two-pair check per group, the records of a failed group re-checked on their weighted points -- and is honoured under exactly the same
 *   condition: from bn254_kzg_params() records per launch on (bn254_set_kzg_params; one knob for both kinds of record).  bn254_kzg_state counts these launches too.
 *   Without the flag honoured bn254_kzg_verify_folded_batch_device only enqueues on hip_stream, and after bn254_kzg_fold_reserve(n', k', device) with k' = k and n' >=
 *   min(n, the records of a pass) it allocates nothing.  A pass holds at most min(2^18, floor(2^18 * 4 / (k + 2)) rounded down to a multiple of 64) records.
 *   Kernels: k_kzg_fold_load (the checks, the transcript hashed straight from the record, the running power of gamma, glv_decompose, k + 2 or k + 3 term records),
 *   then everything bn254_kzg_verify_batch runs behind k_kzg_load.  Measured: profiles/r18_kzg_fold.txt (tools/bench_kzg.py --digests). */
#define BN254_KZG_FOLD_MAX_DIGESTS 13
#define BN254_KZG_FOLD_MAX_DATA 64
#define BN254_KZG_FOLD_LEN(k, data_len) ((size_t)96 + (size_t)96 * (size_t)(k) + (size_t)(data_len))
int bn254_kzg_verify_folded_batch(const uint8_t* key, const uint8_t* records, size_t stride, size_t n, size_t n_digests, size_t data_len, uint8_t* status, int device, unsigned flags);
int bn254_kzg_verify_folded_batch_device(const void* d_key, const void* d_records, size_t stride, size_t n, size_t n_digests, size_t data_len, void* d_status, int device,
                                         void* hip_stream, unsigned flags);
int bn254_kzg_fold_reserve(size_t n, size_t n_digests, int device);

/* ---- Batch G1 multi-scalar multiplication with per-item and shared bases ------------------------------------------------------------------------------------------
 * The G1 work in front of a pairing check, for callers who do not bring a gnark key: the public-input sum IC_0 + sum x_j IC_j of a Groth16 key of one's own (the
 * restated item of bn254_pairing_check_batch_shared needs it), linear combinations of commitments, Pedersen openings, the EVM's ecAdd and ecMul (EIP-196) in bulk.
 *
 *   An ITEM is n_var pairs (point x | y, 64 bytes; scalar, 32 bytes), then n_unit bare points (64 bytes each), then n_shared scalars (32 bytes each): BN254_G1_MSM_ITEM_LEN(v,
 *   u, s) = 96 v + 64 u + 32 s bytes.  Every field is 32-byte big-endian, an all-zero point is the identity.  The shape (n_var, n_unit, n_shared) is the call's: 0 <= n_var
 *   <= BN254_G1_MSM_MAX_VAR, 0 <= n_unit <= BN254_G1_MSM_MAX_UNIT, 0 <= n_shared <= BN254_G1_MSM_MAX_SHARED, one term at least; item_stride >= the item length (bytes behind
 *   the item are ignored).  The limits are the row planner's (csrc/bn254_msm.h: MSM_MAX_FIXED, four unit terms, 32 rows; tests/test_g1_msm_cpu.py walks it over every shape).
 *   ecAdd is the shape (0, 2, 0), ecMul (1, 0, 0).
 *
 *   Result of item i:  S_i = sum_{t < n_var} k_t P_t + sum_{t < n_unit} U_t + sum_{j < n_shared} c_j B_j,  B_j the j-th point of the prepared bases.  out receives 64 bytes
 *   x | y per item, all-zero for the identity and for an item that ends in an error.  status[i], decided in this order (the order of bn254_kzg_verify_batch):
 *     1. with BN254_FLAG_STRICT_SCALARS any scalar of the item >= r is BN254_ERR_NOT_MEMBER (without the flag scalars are used modulo r, as EIP-196 defines ecMul);
 *     2. the points in record order: a coordinate >= p is BN254_ERR_NOT_MEMBER, then a point off the curve BN254_ERR_NOT_ON_CURVE;
 *     3. BN254_ACCEPT: out holds S_i.
 *   A failing item does not disturb its neighbours.  Any other flag is BN254_E_BAD_ARG.
 *
 *   bn254_g1_bases_prepare takes 1 .. BN254_G1_MSM_MAX_SHARED points (64 bytes each), checks them by rule 2 -- *status is BN254_ACCEPT, or the first failure with *out null
 *   and return code BN254_OK, as bn254_kzg_key_prepare does -- builds their 13-bit window tables on `device` (about 13 MB per point; the builder of the PlonK keys) and
 *   returns a handle bound to that device.  The handle is a void* (an opaque owner; bn254_g1_bases_count reads its size, 0 for anything else).  An identity base is
 *   accepted and its terms contribute nothing.  bn254_g1_bases_free waits for the device the handle belongs to, so work enqueued with the handle has finished.  `bases` may
 *   be null exactly when n_shared == 0; a call whose device is not the handle's is BN254_E_BAD_ARG.
 *
 *   Argument errors are BN254_E_BAD_ARG before any device is touched, out and status untouched: null pointers with n > 0, a shape outside the limits or without a term,
 *   a stride below the item length, n_shared above the handle's count, unknown flags.  n == 0 returns BN254_OK.  Lack of memory is BN254_E_NOMEM.  The first use of a
 *   device runs the self-test, as elsewhere; there is no CPU fallback.
 *   bn254_g1_msm_batch stages passes through pinned memory and returns when out and status are back.  bn254_g1_msm_batch_device only enqueues on hip_stream, and after
 *   bn254_g1_msm_reserve(n', the same shape, device) with n' >= min(n, the items of a pass) it allocates nothing.
 *   A PASS holds at most  min(2^18, floor(2^31 / (105 (v + u + s) + 1792 v + 3522)) rounded down to a multiple of 64)  items: per item a term record and flag byte per
 *   term (105 bytes), 1792 bytes of window-table scratch per variable term, up to 32 rows of 108 bytes and 66 bytes of sum, identity flag and loader status -- 2 GiB per
 *   pass at most ((1,0,0) and (2,0,0): 2^18 items; (16,0,0): 63 360).  BN254_G1_MSM_PASS in the environment, read once at load time, lowers it (tests; 64 at least).
 *   Workspace and locking: a per-device workspace of this entry's own -- the buffers of that formula for the largest reservation or call so far, and for the host entry
 *   pinned and device staging of a pass's items and 65 result bytes per item -- with its own lock and completion event: calls on one device serialise among themselves,
 *   and with no other entry (the pairing workspace is not used; the host entry borrows the stream of the pairing batch's host entries, so it adds no stream to the process).
 *   Kernels: k_g1_msm_load (checks, scalars mod r, glv_decompose, term records), k_g1_msm_rows / k_g1_sum_affine (the G1 walk of csrc/bn254_msm.h: variable terms in two-bit
 *   windows -- split, unsplit or joint by the launch's size -- unit terms one mixed addition, shared terms at most 20 mixed additions from the handle's tables),
 *   k_g1_msm_store (64 big-endian bytes and the status byte).
 *   Measured on one MI355X (profiles/r19_g1_msm.txt, tools/bench_g1_msm.py; device-resident valid items, median of 5 calls alternating over the shapes, ms per call at
 *   4096 | 65 536 | 262 144 items):  (1,0,0) 0.68 | 0.98 | 3.73;  (2,0,0) 0.69 | 1.42 | 5.67;  (8,0,0) 0.83 | 4.52 | 20.7;  (16,0,0) 1.12 | 9.82 | 38.0;  (0,2,0) 0.11 |
 *   0.12 | 0.34;  (2,1,0) 0.70 | 1.55 | 5.93;  (0,0,2) 0.27 | 0.30 | 1.04;  (0,0,16) 0.83 | 1.61 | 6.35;  (2,1,16) 0.75 | 3.09 | 13.2.  Beside them in the same session:
 *   bn254_kzg_verify_batch exact minus the pairing alone, which is the (2,1,0) walk behind another loader, 0.70 | 1.56 | 5.39 ms. */
#define BN254_G1_MSM_MAX_VAR 16
#define BN254_G1_MSM_MAX_UNIT 4
#define BN254_G1_MSM_MAX_SHARED 16
#define BN254_G1_MSM_ITEM_LEN(v, u, s) ((size_t)96 * (size_t)(v) + (size_t)64 * (size_t)(u) + (size_t)32 * (size_t)(s))
int bn254_g1_bases_prepare(const uint8_t* points, size_t n_bases, int device, void** out, uint8_t* status);
void bn254_g1_bases_free(void* bases);
size_t bn254_g1_bases_count(const void* bases);
int bn254_g1_msm_batch(const uint8_t* items, size_t item_stride, size_t n_var, size_t n_unit, size_t n_shared, const void* bases, size_t n, uint8_t* out, uint8_t* status,
                       int device, unsigned flags);
int bn254_g1_msm_batch_device(const void* d_items, size_t item_stride, size_t n_var, size_t n_unit, size_t n_shared, const void* bases, size_t n, void* d_out, void* d_status,
                              int device, void* hip_stream, unsigned flags);
int bn254_g1_msm_reserve(size_t n, size_t n_var, size_t n_unit, size_t n_shared, int device);

/* ---- Known-answer self-test of the verdict kernels, per device ----------------------------------------------------------------------------------------------
 * Every verdict comes out of hand-written gfx950 kernels, and the compiler has already produced one wrong build of this code (tools/repro/).  So
 * before a device is first used the library runs the kernels IT SHIPS on THAT device on small built-in inputs and compares every output byte with a known answer.
 *
 * The automatic run happens once per process and device, at the places that make a device ready: the first bn254_groth16_* / bn254_plonk_* / bn254_sp1_* call that
 * touches the device (reservations included: bn254_*_reserve* pay it, so a _device call enqueued after a reservation stays free of synchronous work), the first use
 * of a key list, bn254_groth16_vk_prepare_batch on a device.  Concurrent first calls on one device wait for the one run.  It runs on a stream of its own (of the
 * lowest priority: it takes no hardware queue from the pool the process's other streams share), synchronises with that stream only, and frees everything it
 * allocated before it returns.
 * If a check disagrees the state is sticky: every entry that would launch verification work on that device returns BN254_E_SELFTEST at once, with the recorded text
 * in bn254_last_error(), and writes no status byte -- until an explicit bn254_device_selftest on that device passes.  (A run that could not be made -- no memory, a
 * runtime error -- returns that error and records nothing: the next call tries again.)
 * BN254_SELFTEST=0 in the environment, read once when the library is loaded, skips the automatic run (state 2); the explicit entry still works.
 * BN254_PLONK_SELFTEST and the per-key self-test of the PlonK stage kernels are independent of this and stay as they were.
 *
 * The checks (bit k of a failed mask; the names are part of the interface):
 *    0 fp            the lane Fp product on 64 operand pairs: 0, 1, p - 1, p - 2, all-ones and alternating digits, pseudo-random values
 *    1 fp12_lane     the lane Fp12 kernels: product, square, inverse, cyclotomic square (after the easy part, and on a cyclotomic element), Frobenius 1..3
 *    2 fp12_coop     single operations of the cooperative layout on 6 values (two wavefronts): product, square, 3 cyclotomic squarings, Frobenius 1..3, inverse,
 *                    k_coop12_final_exp
 *    3 pairing_lane  the variable-Q Miller loop and the final-exponentiation program: e(G1, G2), e(aG1, bG2), e(-aG1, bG2) and one more pair
 *    4 g16_lane      the exact Groth16 lane form (k_g16_prepare, k_miller_run, the final exponentiation with its verdict product) through bn254_launch_g16, forced whatever
 *                    BN254_COOP or any knob says: a built-in 2-input key and 64 proofs, valid ones and every corruption class of bn254_synth_groth16; status bytes
 *    5 g16_coop      k_g16_prepare and k_coop12_miller_g16 on the same key and proofs
 *    6 pair2_lane    the lane form of the PlonK pairing check (k_miller_run_fixed2, final exponentiation, k_g16_compare) on the built-in key's two line tables: 64 items,
 *                    accepted ones, rejected ones, items with an identity argument
 *    7 pair2_coop    k_coop12_miller_fixed on the same items
 *    8 codec         k_g16_decompress: 8 compressed proofs, flag 0b00, an x without a square root, the G2 infinity flag
 *    9 sha256        k_sp1_public_inputs: values of 0, 55, 56, 64, 119, 120 and 1000 bytes at unaligned offsets and one range outside the buffer
 * Expected values: the status bytes of checks 4 .. 7 are tables generated with the key's trapdoors (gen_constants.py -> csrc/bn254_constants.h; no pairing is
 * computed for them at run time); everything else is the host's compile of the same arithmetic source, computed once per process while the device runs.
 * NOT covered in this revision: the _keys variants of the kernels (batches over many keys), the RLC group kernels, the MSM row kernels and the wide-key MSM kernels,
 * the kernels of the batch pairing product (k_pairing_load, k_miller_run_var, k_pairing_store, and k_pairing_load_shared, k_miller_run_mix of the entries with shared G2 points; its final exponentiation and
 * compare are checks 1 .. 3's kernels), the kernels of its BN254_FLAG_RLC mode (k_pairing_rlc_weigh, k_miller_run_sub, k_pairing_rlc_group_sums, k_pairing_rlc_group_prod),
 * the kernels of the KZG batch (k_kzg_load, k_kzg_fold_load, k_kzg_ident, k_kzg_fetch),
 * the table builders (the window tables of the built-in key are built on the device, so a wrong table fails checks 4 and 5, but no table is compared).
 * Nor does a run of it see the PlonK stage kernels: those have the per-key self-test -- one synthetic proof, lane 0 of workgroup 0, ChaCha20 blocks 0 .. 2 -- and, in the
 * test suite, a batch-wide value test (bn254_dbg_plonk_stages, tests/test_gpu_plonk_stage_values.py) that holds every lane's zeta, lambda, opening, hash-to-field values and
 * pairing operands, the lambda stream (blocks 3i .. 3i + 2 per slot) and the weight stream of BN254_FLAG_RLC to the oracle, under one key and over key lists.
 *
 * Cost on one MI355X (profiles/selftest_cost.txt): one run is 40 ms of wall time in a warm process, all of it device time on the run's own stream (g16_lane 11.2 ms,
 * pairing_lane 9.0, pair2_lane 8.3, g16_coop 1.9, the built-in key's window tables 1.5, codec 1.4, pair2_coop 1.3, fp12_coop 1.1, fp12_lane 0.7); the host's share (the key
 * 3 ms, the expected values 7.8 ms, once per process) runs while the device works.  A process's first single-proof bn254_groth16_verify -- runtime initialisation, code
 * objects, key preparation -- took 261 ms (median of five processes) before this feature, 295 ms with the automatic run, 270 ms with BN254_SELFTEST=0.
 *
 * bn254_device_selftest: runs all checks NOW on `device`, whatever ran before and whatever the environment says.  *failed_mask: bit k set when check k disagrees;
 *   *ms: the wall time of the run; either may be null.  BN254_OK when every check agrees; BN254_E_SELFTEST when one does not -- bn254_last_error() then names the first
 *   failing check and gives a short hex prefix of the device's value and of the expected one; BN254_E_NO_DEVICE / BN254_E_BAD_ARG / BN254_E_HIP / BN254_E_NOMEM as
 *   everywhere.  Its result REPLACES the device's recorded state: a pass clears an earlier failure.  An operator's health check.
 * bn254_device_selftest_state: *state = -1 (not run yet), 0 (failed), 1 (passed), 2 (skipped: BN254_SELFTEST=0); *failed_mask (may be null): the mask of the recorded
 *   run.  Touches no device.
 * bn254_selftest_check_name: the name of check 0 .. 9, "" outside. */
#define BN254_SELFTEST_NUM_CHECKS 10
int bn254_device_selftest(int device, unsigned* failed_mask, float* ms);
int bn254_device_selftest_state(int device, int* state, unsigned* failed_mask);
const char* bn254_selftest_check_name(int check);

/* ---- measurement support ------------------------------------------------------------------------------------------
 * A sub-batch above COOP12_MAX_PROOFS runs as about 110 kernel launches: k_g16_prepare, the whole Miller loop as ONE k_miller_run (or a few, g16_launch_form; the
 * first sets f and T, the last tests B's subgroup) and one launch per Fp12-level operation of the final exponentiation (k_f12_mul x 54, the last of them with the
 * comparison as its tail, k_f12_cyclo_sqr_n x 36, ...); up to COOP12_MAX_PROOFS as two (k_g16_prepare, the cooperative kernel).  When profiling is enabled, verify_batch_device records HIP
 * events on the launch stream (a) at the four phase boundaries (prepare | subgroup | Miller loop | final exponentiation) and
 * (b) around every launch whose kernel kind is selected by bn254_set_profile_kernels (bit i = kind i, default all).
 * After the stream has been synchronised bn254_groth16_last_kernel_ms returns the phase durations and
 * bn254_groth16_kernel_profile the number of launches and the summed duration per kernel kind, together with the number of
 * proofs each launch covered (the first sub-batch when the batch is split over concurrent streams, BN254_STREAMS).
 * bn254_set_profiling: 0 off; 1 the event pairs of (b) are those of the LAST batch; 2 they accumulate over every batch enqueued since the last call of one of the
 * two setters (up to 1024 launches per sub-batch stream, further ones are not recorded), so that a caller timing back-to-back batches reads them once, after its
 * final synchronisation, instead of waiting for each batch. */
#define BN254_G16_NUM_KERNELS 4   /* phases */
void bn254_set_profiling(int enabled);
void bn254_set_profile_kernels(unsigned mask);
int bn254_groth16_last_kernel_ms(const bn254_g16_pvk* pvk, int device, float ms[BN254_G16_NUM_KERNELS]);
int bn254_groth16_rlc_state(const bn254_g16_pvk* pvk, int device, float* fallback_share, unsigned* bypassed_calls);   /* BN254_FLAG_RLC, adaptive use */
/* A large batch runs as two sub-batches on two streams; the HIP runtime maps the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4) and
 * streams that share a queue run one after the other.  The library does not touch the environment (the number of queues is a deployment setting);
 * it measures: a two-stream batch of a (key, device) is bracketed with events, a later call reads them.  overlap = sum of the two sub-batches' durations /
 * their union (~2 side by side, ~1 one after the other; -1 not measured yet).  One measurement decides nothing (another tenant's kernels, a tool that serialises dispatches):
 * three in a row must read "one after the other" before single_stream = 1 (batches that fit one launch then run as one sub-batch), one that reads "side by side" settles it
 * the other way; on single_stream every 256th batch runs two sub-batches again and is measured, so a transient cause does not pin the key to the slower plan.  The one-line
 * explanation is kept per (key, device): this call copies it to the calling thread's bn254_last_diagnostic(). */
int bn254_groth16_stream_overlap(const bn254_g16_pvk* pvk, int device, float* overlap, int* single_stream);
const char* bn254_last_diagnostic(void);
/* Knobs of BN254_FLAG_RLC (process-wide, atomics; a negative argument leaves that knob alone): the batch size from which the flag is honoured
 * (default 200 000, never below 64), the adaptive bypass on / off, and the lanes a launch part must keep for its proofs to share Miller-loop
 * accumulators (default 65536).  The environment variables BN254_RLC_MIN_BATCH / BN254_RLC_ADAPTIVE / BN254_RLC_SHARE_MIN_LANES give the
 * initial values and are read once, when the library is loaded. */
void bn254_set_rlc_params(long min_batch, int adaptive, long share_min_lanes);
const char* bn254_groth16_kernel_name(int i);                 /* phase names */
int bn254_groth16_num_kernel_kinds(void);
const char* bn254_groth16_kernel_kind_name(int i);
int bn254_groth16_kernel_profile(const bn254_g16_pvk* pvk, int device, unsigned launches[], float total_ms[], size_t* proofs_per_launch);
/* Same over the first TWO sub-batches (two streams side by side), plus union_ms[kind]: the length of the union of the launch intervals of that kind
 * on a common time base.  Work of all the launches / union = the rate the GPU delivered while that kernel kind ran, whether the two streams' launches
 * overlapped (union = about one launch) or ran one after the other (union = the sum). */
int bn254_groth16_kernel_profile_all(const bn254_g16_pvk* pvk, int device, unsigned launches[], float total_ms[], float union_ms[], size_t* proofs_per_launch);

/* ---- synthetic gnark-format workload generator (bench / tests; host threads, no GPU) --------------------------------
 * Deterministic (SplitMix64 seed).  Writes a gnark-compressed verifying key (292 + 32 (n_public+1) + 4 + 128 bytes), n
 * proofs (256 bytes each, A | B | C uncompressed) that satisfy gnark's equation, their public inputs, and the status the
 * verifier must return.  If invalid_every > 0 every invalid_every-th proof is corrupted, cycling through: public input
 * + 1 (REJECT), C + G1 (REJECT), A.y + 1 (NOT_ON_CURVE), B replaced by a twist point outside G2 (NOT_IN_SUBGROUP),
 * A.x >= p (NOT_MEMBER).  agree bit 0: the key is sampled so that BN254_VK_REFERENCE and BN254_VK_GNARK agree on it; bit 1:
 * every proof with index = 3 (mod 7) gets a last public input that makes L = K0 + sum x_i K_i the identity (still a valid proof). */
size_t bn254_synth_groth16_vk_len(size_t n_public);
int bn254_synth_groth16(uint64_t seed, size_t n_public, size_t n, int invalid_every, int agree, int threads,
                        uint8_t* vk_out, uint8_t* proofs_out, uint8_t* inputs_out, uint8_t* expected_status_out);
/* proofs [first, first + n) of the same stream (proof i depends on (seed, i) only), written to positions 0 .. n-1: a rank of a sharded job
 * generates just its own contiguous shard; the key is the same for every range */
int bn254_synth_groth16_range(uint64_t seed, size_t n_public, size_t first, size_t n, int invalid_every, int agree, int threads,
                              uint8_t* vk_out, uint8_t* proofs_out, uint8_t* inputs_out, uint8_t* expected_status_out);
/* the key of bn254_synth_groth16(seed, n_public, .., agree = 1, ..) and, for n given input rows (n x n_public x 32 bytes, big-endian, used modulo r), one valid
 * 256-byte raw proof per row: the SP1 tests need proofs for inputs they cannot choose (a digest) */
int bn254_synth_groth16_for_inputs(uint64_t seed, size_t n_public, size_t n, const uint8_t* inputs, int threads, uint8_t* vk_out, uint8_t* proofs_out);

/* ---- synthetic PlonK workload generator (bench / tests; host threads, no GPU) ----------------------------------------
 * Deterministic (SplitMix64 seed).  Writes a verifying key in the reference's layout (plonk/converter.rs:18-119; bn254_synth_plonk_vk_len(n_qcp) = 34 328 + 40 n_qcp
 * bytes, the skipped 33 788 bytes zero) with n_public public inputs, n_qcp BSB22 commitments (at most 8) and a domain of 2^log2_size rows (1..28, at least
 * n_public + n_qcp), n DISTINCT proofs that the verifier accepts (bn254_synth_plonk_proof_len(n_qcp) = 808 + 96 n_qcp bytes each, at proof_stride bytes from one
 * another; a record is zero past its proof), their public inputs (n x n_public x 32 bytes, canonical) and the status the verifier must return.  The proofs come from
 * the KZG secret, which the generator draws with the key: it opens random commitments to random claimed values.  If invalid_every > 0 every
 * invalid_every-th proof is corrupted, cycling through: public input 0 + 1 (OPENING_MISMATCH), the shifted opening proof + G1 (PAIRING_FAILED), L.y + 1
 * (NOT_ON_CURVE), Z.x >= p (NOT_MEMBER), the first commitment's claimed selector value + 1 (PAIRING_FAILED), the last commitment dropped (BSB22_MISMATCH).  A class
 * the key has nothing for (no inputs: the first; no commitments: the last two) becomes the second.  The key is a function of (seed, n_public, n_qcp, log2_size)
 * alone, proof i of (seed, i) and the key.  BN254_E_BAD_ARG (nothing written): n_qcp > 8, log2_size outside 1..28, a domain smaller than n_public + n_qcp,
 * proof_stride below the proof length, a null buffer that would be written. */
size_t bn254_synth_plonk_vk_len(size_t n_qcp);
size_t bn254_synth_plonk_proof_len(size_t n_qcp);
int bn254_synth_plonk(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, size_t n, int invalid_every, int threads,
                      uint8_t* vk_out, uint8_t* proofs_out, size_t proof_stride, uint8_t* inputs_out, uint8_t* expected_status_out);
/* proofs [first, first + n) of the same stream, written to positions 0 .. n-1; the key is the same for every range */
int bn254_synth_plonk_range(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, size_t first, size_t n, int invalid_every, int threads,
                            uint8_t* vk_out, uint8_t* proofs_out, size_t proof_stride, uint8_t* inputs_out, uint8_t* expected_status_out);
/* the key of bn254_synth_plonk for the same arguments and, for n given input rows (n x n_public x 32 bytes, big-endian, each below r: BN254_E_BAD_ARG otherwise),
 * one valid proof per row: the SP1 entry needs proofs for inputs the caller cannot choose (a digest) */
int bn254_synth_plonk_for_inputs(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, size_t n, const uint8_t* inputs, int threads,
                                 uint8_t* vk_out, uint8_t* proofs_out, size_t proof_stride);

/* ---- probes of the device arithmetic, used by the GPU parity tests (tests/test_gpu_*.py) ---------------------------
 * Each runs one lane per item on `device` and copies the result back.  Fp12 layout: 12 x 32 bytes in tower order
 * c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1; G1: x | y; G2: x.c1 | x.c0 | y.c1 | y.c0 (gnark order). */
/* measurement probe: lane-level v_mad_u64_u32 per second of `device` (four wavefronts per SIMD, launches of about 2 ms, 16 independent chains per lane): the VALU peak of THIS box */
int bn254_dbg_valu_peak(int device, double* mads_per_s);
/* the same kernel back to back for about ms_target (<= 2000) milliseconds, timed as one interval: the rate the box SUSTAINS over the length of the path's long kernels */
int bn254_dbg_valu_peak_sustained(int device, double ms_target, double* mads_per_s);
int bn254_dbg_fp_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int device);                 /* n x 32 B each */
int bn254_dbg_fp12_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int device);        /* 0 mul 1 sqr 2 inv 3 cyclo_sqr(after easy part) 4 frob1 */
int bn254_dbg_pairing(const uint8_t* g1, const uint8_t* g2, uint8_t* out_gt, size_t n, int device);          /* e(P_i, Q_i), n x 384 B */
/* The batch pairing product (bn254_pairing_check_batch above; same arguments and argument errors) with a choice of where it runs: status[i] as
 * bn254_pairing_check_batch defines it AND, when out_gt is non-null, the GT value of every item that reached the pairing as bn254_pairing_batch writes it, from one
 * run.  device -1: the HOST compile of the same loader, Miller run (vm_miller_run_var) and final-exponentiation program on a plain-array accessor, no device is
 * touched; a device ordinal: the kernels. */
int bn254_dbg_pairing_batch(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* out_gt, uint8_t* status, int device);
/* The same with the form of every launch forced: form 0 is bn254_dbg_pairing_batch; 1 (the lane kernels) and 2 (the cooperative kernel) need a device ordinal, and
 * form 2 takes at most 30 720 items -- otherwise BN254_E_BAD_ARG with the buffers untouched. */
int bn254_dbg_pairing_batch_form(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* out_gt, uint8_t* status, int device, int form);
/* the form a launch of n items of n_pairs pairs takes under the knobs as they are now: *form = 1 lane, 2 cooperative; no device is touched */
int bn254_dbg_pairing_form(size_t n_pairs, size_t n, int* form);
/* The same probe for items with shared, prepared G2 points (bn254_pairing_check_batch_shared: same arguments and argument errors): device -1 with form 0 runs the
 * host compile of k_pairing_load_shared, k_miller_run_mix and the final-exponentiation program, the loop cut by BN254_MILLER_RUN_STEPS; a device ordinal runs the
 * kernels with form 0 (the plan), 1 (lane) or 2 (cooperative). */
int bn254_dbg_pairing_batch_shared(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared,
                                   size_t n, uint8_t* out_gt, uint8_t* status, int device, int form);
/* host-only probe of its pass plan for a call of n items of n_pairs pairs: out = {items a reservation of n allocates workspace for, items per pass of the host
 * entries, passes of the host entries, pinned bytes of the records of one pass} */
int bn254_dbg_pairing_plan(size_t n_pairs, size_t n, uint64_t out[4]);
/* test-only: BN254_FLAG_RLC on the pairing batch is honoured for shapes of at most max_var variable positions (0 .. 8; negative: the default, 0); returns the value
 * it replaces */
int bn254_dbg_set_pairing_rlc_max_var(int max_var);
/* The probe of BN254_FLAG_RLC on the pairing batch (bn254_pairing_check_batch_flags: same items, records and argument errors; one pass): ONE weighted launch whatever
 * the knob says, with the caller's weights (n x 16 bytes big-endian, forced odd; null: the real draw on a device, all 1 in the host compile) in the ChaCha20 stream's
 * place, so that every value is checkable.  out_item_gt (null, or n x 384): the final-exponentiated value of every item that reached the groups, on its weighted points
 * (zero for an item decided before); out_group_gt (null, or ceil(n / 64) x 384) and out_group_status (null, or one byte per group): the value and the verdict of every
 * group (1 and BN254_ACCEPT for a group without a pending item); status: what the entry answers.  device -1 (form 0) runs the host compile of the same code (the weight
 * step, the Miller run over the variable positions, the group sums and product, the group check); a device ordinal the kernels, with the group check and the exact check
 * in form 0 (the plan), 1 (lane) or 2 (cooperative). */
int bn254_dbg_pairing_batch_rlc(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared, size_t n, const uint8_t* weights,
                                uint8_t* out_item_gt, uint8_t* out_group_gt, uint8_t* out_group_status, uint8_t* status, int device, int form);
/* The probe of the KZG batch (bn254_kzg_verify_batch: same key, openings and argument errors; one pass: n at most what a launch holds): the points the loader and the
 * G1 walk leave per opening -- out_f: vp_p(0), F_i or F'_i; out_h: vp_p(1), -H_i or H'_i = -r_i H_i; 64 big-endian bytes each, zero for the identity and for an opening
 * the loader decided; out_inf: their two identity flags -- and the status bytes of the check.  flags may carry BN254_FLAG_RLC: then the weighted path runs whatever the
 * knob says, with the caller's weights (n x 16 bytes, big-endian, forced odd; null: all 1) in the ChaCha20 stream's place, so that every value is checkable; out_group
 * (null, or groups x 131 bytes) receives per group of 64 openings the two sums, their identity flags and the group's status byte (BN254_ACCEPT, BN254_REJECT).
 * weights and out_group need BN254_FLAG_RLC.  device -1 (form 0) runs the host compile of the same code (kzg_load_opening, the rows of the plan, the group sums, the
 * mixed Miller run); a device ordinal the kernels, with the pairing launches in form 0 (the plan), 1 (lane) or 2 (cooperative). */
int bn254_dbg_kzg_fold(const uint8_t* key, const uint8_t* openings, size_t stride, size_t n, const uint8_t* weights, unsigned flags, uint8_t* out_f, uint8_t* out_h,
                       uint8_t* out_inf, uint8_t* out_status, uint8_t* out_group, int device, int form);
/* ... and of the batch-opening records (bn254_kzg_verify_folded_batch: same arguments and argument errors): everything bn254_dbg_kzg_fold writes, and out_fold, n x 64
 * bytes: per record the 32-byte digest gamma is reduced from, then y^ = sum gamma^i y_i as 32 canonical big-endian bytes (all zero for a record the loader decided). */
int bn254_dbg_kzg_fold_proof(const uint8_t* key, const uint8_t* records, size_t stride, size_t n, size_t n_digests, size_t data_len, const uint8_t* weights, unsigned flags,
                             uint8_t* out_fold, uint8_t* out_f, uint8_t* out_h, uint8_t* out_inf, uint8_t* out_status, uint8_t* out_group, int device, int form);
/* host only: BN254_OK iff the G1 walk of n records of n_digests digests plans (weighted: the BN254_FLAG_RLC shape) within lane_budget lanes (0: the library's) and joint
 * rows of joint_g terms (negative: the library's choice for n); *rows (optional): the rows of the plan */
int bn254_dbg_kzg_fold_plan(size_t n_digests, int weighted, size_t n, size_t lane_budget, int joint_g, int* rows);
/* Value-level probes of the Fp12 operations (tests).  An Fp12 value travels in one of two formats, twelve Fp numbers in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ..):
 *   format 0  384 bytes, 32 big-endian canonical bytes per number;
 *   format 1  108 int32: per number the nine balanced 29-bit digits (digit 0 first) of a representative of its Montgomery form x 2^261 mod p, stored into
 *             and read from the workspace AS GIVEN -- the caller chooses the representative and must stay inside the operation's input contract
 *             (the eight low digits in [-2^28, 2^28], |value| <= 2.42 p).
 * bn254_dbg_fp12_op_fmt: the lane kernels; op as bn254_dbg_fp12_op and 5 cyclo_sqr 6 frob2 7 frob3 8 a conj(b) 9 conj(a) b (the conjugations as the kernels fuse them).
 * bn254_dbg_coop12_op: ONE operation of the cooperative layout (csrc/bn254_coop12.hip), five proofs per wavefront, called as the product calls it.  For the
 * line products b is the Fp12 d0 + d3 w + d4 w^3 (every other coefficient zero; d0 in Fp for ops 8 and 9); arg: the squaring count (1 .. 64) or the Frobenius power (1 .. 3).
 * op of bn254_dbg_coop12_op: 0 a b; 1 a conj(b) (conj_b of c12_mul); 2 conj(a) b (a flagged VE_CONJ, rewritten by Coop12Ops); 3 general squaring; 4 cyclotomic
 * squarings, arg of them; 5 Frobenius, power arg; 6 inverse; 7 conjugate; 8 c12_mul_line_fp; 9 the same with keep (the line counts as 1: a is returned);
 * 10 c12_mul_line_fp2; 11 k_coop12_final_exp. */
int bn254_dbg_fp12_op_fmt(int op, const void* a, const void* b, void* out, size_t n, int in_format, int out_format, int device);
int bn254_dbg_coop12_op(int op, const void* a, const void* b, void* out, size_t n, int in_format, int out_format, int arg, int device);
/* The compares that decide a verdict, on values the caller places: n values a (and b), ONE target of twelve numbers in format 0; out_status: n bytes,
 * BN254_ACCEPT or BN254_REJECT.  form 0: k_g16_compare (a == target); 1: k_f12_mul_verdict (a b == target, compared as the product is stored);
 * 2: c12_eq_const of the cooperative kernels (a == target).  (k_f12_mul_verdict_keys takes its target from a key set's descriptors: it has no probe.) */
int bn254_dbg_verdict(int form, const void* a, const void* b, const uint8_t target[384], uint8_t* out_status, size_t n, int in_format, int device);
/* The cooperative kernels in their store modes, with the line tables of a prepared key (gamma side: table 0, delta side: table 1; bn254_groth16_vk_prepare says
 * which signs they hold).  _fixed: k_coop12_miller_fixed without a target (its store mode) on n_pairs (1 or 2) table-driven pairs: g1_0 / g1_1 n x 64 bytes
 * (g1_1 unused for one pair), identity: null or n bytes, bit t = the G1 point of pair t is the identity (its bytes are then ignored); out_gt n x 384 bytes.
 * _g16: k_g16_prepare and k_coop12_miller_g16 (store mode: no target) on n raw 256-byte proofs with their inputs (keys with at most 16 inputs);
 * out_status[i]: BN254_ACCEPT where the proof reached the pairing and out_gt holds its value, else the loader's status (out_gt is then unspecified). */
int bn254_dbg_coop12_miller_fixed(const bn254_g16_pvk* pvk, int n_pairs, const uint8_t* g1_0, const uint8_t* g1_1, const uint8_t* identity, uint8_t* out_gt, size_t n, int device);
int bn254_dbg_coop12_miller_g16(const bn254_g16_pvk* pvk, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_public, size_t n, uint8_t* out_gt, uint8_t* out_status,
                                int device);
/* The Groth16 loader stage by value: what a batch's launches leave in the workspace BEFORE the pairing -- A, B, C as parsed and L = K_0 + sum x_j K_j -- through
 * the product's own launcher of the stage (csrc/bn254_kernels.hip, bn254_launch_g16_loader: k_g16_classify / k_g16_compact_write, k_g16_prepare, k_g16_check_scalars,
 * and for a key with more than 16 inputs the digit, partial-sum and reduction launches).  Every argument is checked on the host before a device is looked at
 * (BN254_E_BAD_ARG); n is at most 32 768.
 * bn254_dbg_g16_loader: n raw 256-byte records at proof_stride and n rows of n_public inputs under one prepared key.
 *    flags       0 or BN254_FLAG_STRICT_SCALARS
 *    form        what the sizes and knobs would otherwise decide: 0 the lane form, L by the whole k_g16_prepare; 1 the same on compacted slots; 2 wide, the chunk sums
 *                added by k_g16_msm_reduce; 3 wide, by k_g16_msm_reduce8.  A combination no launch of the product takes is refused: forms 0 / 1 with a key of more
 *                than 16 inputs and its own input count, forms 2 / 3 with any other key or count, form 1 under BN254_FLAG_STRICT_SCALARS, form 3 with fewer than 16
 *                chunk sums per proof.  (Form 2 at 16 chunks and more is what the product launches above 65 536 proofs.)  Comb or byte-window tables: as the key was
 *                prepared.
 *    misalign    0 .. 3: the device copy of the input rows starts that many bytes past a 4-byte boundary (the kernels' byte-wise load branch)
 *    out_status  n bytes, the caller's status buffer as the stage leaves it: per proof a final loader status, or BN254 internal PENDING (0x80) | 0x40 when L is the
 *                identity | the deferred status of C.  Form 1: what k_g16_classify left (final, or 0x80), and the slots' bytes in out_slot_status
 *    out_slot_status, out_slot_proof   form 1 only (else unused, may be null): n slot status bytes (0 past the pending proofs) and n slot -> proof words
 *    out_points  n x 320 bytes, per proof (form 1: per slot) A (64) | B (128: x.c1 x.c0 y.c1 y.c0) | C (64) | L (64; (0, 1) for the identity), canonical big-endian
 *                values of the workspace elements; meaningful where the status byte is pending
 *    info        what the launcher recorded at its launch sites as it enqueued them (not the request echoed): {form that ran (0 .. 3 as above; -1: none of them),
 *                chunk sums per proof (0: not wide), reduction kernel (0 none, 1 k_g16_msm_reduce, 2 k_g16_msm_reduce8), partial-sum kernel (0 none: L by
 *                k_g16_prepare's 13-bit windows, 1 k_g16_msm_partial_comb, 2 k_g16_msm_partial), k_g16_check_scalars launched, k_g16_comb_digits launched}
 * bn254_dbg_g16_loader_keys: the same stage of a batch over a key list in its grouped form (the grouping launches, then k_g16_prepare_keys and under the strict
 *    flag k_g16_check_scalars_keys over all slots as one launch part); arguments as bn254_groth16_verify_batch_keys.  Per slot: out_slot_proof (all ones in a padding
 *    slot), out_slot_status (0 there), out_points as above; the arrays hold max_slots entries (the batch's slots: every key's count rounded up to 64), *out_n_slots
 *    receives the count the device found. */
int bn254_dbg_g16_loader(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n, unsigned flags, int form,
                         int misalign, uint8_t* out_status, uint8_t* out_slot_status, unsigned* out_slot_proof, uint8_t* out_points, int info[6], int device);
int bn254_dbg_g16_loader_keys(const bn254_g16_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                              size_t input_stride, size_t n, unsigned flags, int misalign, size_t max_slots, unsigned* out_slot_proof, uint8_t* out_slot_status, uint8_t* out_points,
                              size_t* out_n_slots, int device);
/* The G1 layer of the PlonK path by value (csrc/bn254_k_msm.hip), through the product's own launchers; layouts are converted on the host.  Every argument is checked
 * before anything is launched (BN254_E_BAD_ARG: null pointers, indices outside their lists, n = 0 or above the probe's cap, more rows than MSM_MAX_ROWS = 32, coordinates
 * that are not canonical, digits outside the contract), and before the device is looked at.  Points are 64 bytes x | y big-endian; the identity never travels as bytes.
 * bn254_dbg_g1_msm: ONE launch of k_g1_msm_rows (n_keys = 1) or k_g1_msm_rows_keys (n_keys > 1) over n items (at most 32 768) and the row sum after it, planned by
 * msm_plan_build(shape, round_up(n, 64), lane_budget (0: the library's), joint_g) as the PlonK path plans its launches.
 *    shape       shape_ints ints: n_sums | per sum n_var, n_unit, n_fixed | per sum its variable terms, unit terms, fixed terms, the fixed terms' table indices
 *    terms       n x n_terms records of 129 bytes: point (64) | k1 (16, big-endian) | k2 (16) | scalar (32, LITTLE-endian: the eight canonical words of a fixed term) |
 *                flag byte (bit 0: the point is the identity, bits 1 / 2: the signs of k1 / k2; a unit term's sign is bit 1).  n_terms at most 64.
 *    bases       n_keys x n_bases curve points: the window tables of key k are built on the device from bases[k * n_bases ..] (n_bases <= 32, n_keys <= 8)
 *    granule_key n_keys > 1: one key index per 64 items (ceil(n / 64) words)
 *    out_mode 0  out_points receives n x n_sums points (item-major; zero bytes where out_inf says identity), out_inf n x n_sums bytes (1: identity).  Two sums are
 *                added up by one launch of k_g1_sum_affine each (its words form holds one sum per item)
 *    out_mode 1  the call of the second PlonK launch: both sums in one launch into workspace elements VE_LX / VE_CX with BN254_ST_LINF / _LINF2 OR-ed into `status`
 *                (n bytes, the caller's on entry, the kernel's on return); out_points receives n x 2 points as stored: (x, y) of VE_LX, then of VE_CX; out_inf unused
 *    info        {rows, rows with a window table, rows of sum 0, rows of sum 1, form (0 split, 1 unsplit, 2 joint rows), longest row in the planner's units}
 * bn254_dbg_g1_sum_rows: k_g1_sum_affine alone on count_a + count_b (count_b = 0: one sum) rows of n projective points the caller places (n at most 65 536):
 *    rows        row r, item i at index r * n + i.  format 0: 96 bytes X | Y | Z, big-endian canonical field values; format 1: 27 int32, the nine digits of X, of Y and of
 *                Z, stored as given -- inside what the kernel declares for a row it loads: the eight low digits in [-2^28, 2^28], |value| <= 3 p per coordinate
 *    outputs     as above (out_mode 0: n x (1 or 2) points; out_mode 1: n x 2 points and `status`)
 * bn254_dbg_plonk_group_sums: k_plonk_group_sums on n pairs of affine points p0 / p1 (at VE_LX / VE_CX of n proofs, n at most 65 536) with the caller's n status
 * bytes: out_p0 / out_p1 receive the ceil(n / 64) group points as stored, out_group_status the groups' status bytes.  group_verdicts != null: k_plonk_group_scatter
 * then runs with THESE ceil(n / 64) bytes as the groups' status; status_out receives the n status bytes after it and *n_failed its count. */
int bn254_dbg_g1_msm(const int* shape, size_t shape_ints, const uint8_t* terms, size_t n_terms, const uint8_t* bases, size_t n_bases, size_t n_keys, const unsigned* granule_key,
                     size_t n, size_t lane_budget, int joint_g, int out_mode, uint8_t* out_points, uint8_t* out_inf, uint8_t* status, int info[6], int device);
int bn254_dbg_g1_sum_rows(const void* rows, int format, int count_a, int count_b, size_t n, int out_mode, uint8_t* out_points, uint8_t* out_inf, uint8_t* status, int device);
int bn254_dbg_plonk_group_sums(const uint8_t* p0, const uint8_t* p1, const uint8_t* status, size_t n, uint8_t* out_p0, uint8_t* out_p1, uint8_t* out_group_status,
                               const uint8_t* group_verdicts, uint8_t* status_out, unsigned* n_failed, int device);
int bn254_dbg_g2_subgroup(const uint8_t* g2, uint8_t* out_flags, size_t n, int device);                       /* 1 = in G2 (gnark's psi relation, one kernel) */
int bn254_dbg_g2_subgroup_ate(const uint8_t* g1, const uint8_t* g2, uint8_t* out_flags, size_t n, int device); /* 1 = in G2: the product's test, from the Miller loop's final point (g1: any G1 points) */

/* The vectors of the device self-test and a run with a fault injected (tests).
 * bn254_dbg_selftest_vectors (host only): the inputs and the expected outputs of check k.  *in_len / *exp_len are always written; BN254_E_BAD_ARG if a buffer is too small.
 * Layouts (Fp12: 384 bytes, G1: 64, G2: 128, as above):
 *    0  in a[64] | b[64], 32 bytes each                                      expect 64 products
 *    1  in a[2] | b[2] | c[2] (c cyclotomic)                                 expect 8 x 2 values: a b, a^2, 1/a, cyclo_sqr(easy(a)), frob1 a, cyclo_sqr(c), frob2 a, frob3 a
 *    2  in a[6] | b[6] | c[6]                                                expect 8 x 6 values: a b, a^2, c^(2^3), frob1 a, frob2 a, frob3 a, 1/a, final_exp(a)
 *    3  in g1[4] | g2[4]                                                     expect 4 GT values
 *    4, 5  in vk (520 bytes, gnark) | 64 raw proofs | 64 rows of 2 inputs    expect 64 status bytes (key mode BN254_VK_REFERENCE)
 *    6, 7  in Q_0 | Q_1 | target (GT) | P_0[64] | P_1[64] | 64 flag bytes (bit t: P_t is the identity, its bytes are then x = 0, y = 1)
 *                                                                            expect 64 status bytes: BN254_ACCEPT where e(P_0, Q_0) e(P_1, Q_1) = target, else BN254_ERR_PAIRING_FAILED
 *    8  in 11 compressed records of 128 bytes                                expect 11 raw records of 256 bytes | 11 pre bytes (1: does not decompress)
 *    9  in 8 vkey hashes | 9 offsets (u64 LE) | pv_bytes (u64 LE) | the values' buffer (1424 bytes)     expect 8 rows (vkey hash | digest) | 8 pre bytes (1: range outside)
 * bn254_dbg_selftest: the run of bn254_device_selftest with one bit of the DEVICE-SIDE INPUT of check corrupt_check flipped before the upload (-1: none), the expected
 * values untouched: the kernels honestly compute something else -- wrong values, never a fault -- and the comparison must see it (for the status checks the bit changes
 * a proof's status).  record 0: the device's recorded state is not touched; 1: the result is recorded as the automatic run's would be.
 * bn254_dbg_selftest_ms: of the last run in this process: the time between the events around each check (gpu_ms[0 .. 9]; gpu_ms[10]: the built-in key's upload and
 * window tables), the host time spent on the key and the expected values meanwhile, and the run's wall time. */
int bn254_dbg_selftest_vectors(int check, uint8_t* in, size_t in_cap, size_t* in_len, uint8_t* expect, size_t exp_cap, size_t* exp_len);
int bn254_dbg_selftest(int device, int corrupt_check, int record, unsigned* failed_mask);
int bn254_dbg_selftest_ms(float gpu_ms[BN254_SELFTEST_NUM_CHECKS + 1], float* host_ms, float* wall_ms);

/* stage 1 of the PlonK path as the DEVICE runs it (csrc/bn254_k_plonk.hip), for n proofs: zeta -- the last of the four chained Fiat-Shamir challenges
 * (plonk/verify.rs:62-95), 32-byte big-endian, canonical -- and the stage's status per proof (BN254_ACCEPT: alive; else the error it decided) */
int bn254_dbg_plonk_stage1(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n,
                           uint8_t* zeta_out, uint8_t* status_out, int device);
/* Both stages and both MSMs of the PlonK path as the product runs them -- the first part of its one pass, stage 1 -> digest MSM -> stage 2 -> KZG MSM, up to the operands of
 * the pairing check -- under a ChaCha20 key the CALLER gives (lam_key: 8 key words, 3 nonce words), for n <= 4096 proofs; tests/test_gpu_plonk_stage_values.py holds every
 * value to the oracle.  The public entries cannot be given a key: they draw a fresh one per pass.  The arguments are those of bn254_plonk_verify_batch (of
 * bn254_plonk_verify_batch_keys for the list form); of flags only BN254_FLAG_RLC is looked at, and it forces the weighted form whatever the batch size: every scalar of both
 * sums times the proof's weight, 128 bits of the key's second stream (nonce word 2 xor "RLC"), forced odd.  Every argument error is BN254_E_BAD_ARG before a device is touched.
 * out: n records of 560 bytes in proof order, field values 32-byte canonical big-endian, points x | y:
 *     0  the stage-1 status (BN254_ACCEPT: alive, else the error the stage decided)
 *     1  the status after stage 2: BN254_ACCEPT for a proof that reached the pairing check, else the error
 *     2  1: the linearised-polynomial digest is the identity      3  1: P0 is the identity      4  1: P1 is the identity      5 .. 7  zero
 *     8  the slot the proof was given, u32 little-endian (its own index under one key): lambda is drawn from blocks 3 slot .. 3 slot + 2, the weight from block slot
 *    12 .. 15 zero
 *    16  zeta      48  lambda, the KZG batching scalar      80  lin_opening, the value stage 1 computed for the opening of the linearised polynomial
 *   112  the linearised-polynomial digest, the first MSM's result (no oracle call gives it: it localises a wrong P0)
 *   176  hash_to_field of the BSB22 commitments, 8 x 32 bytes, the key's n_qcp first ones used
 *   432  P0      496  P1: the G1 operands of e(P0, g2[0]) e(P1, g2[1]) == 1 as the second MSM stored them (zero for the identity)
 * Everything but the two status bytes and the slot is zero for a proof the stages decided, except zeta on an opening mismatch (as bn254_dbg_plonk_stage1).
 * device -1 (one key only) touches no device: the host compile of the same stage source, lambda and the weight derived as the per-key self-test restates them, and each
 * sum added up term by term with the host's G1 arithmetic, without a plan or tables -- what proves the tests' expectations where there is no GPU. */
int bn254_dbg_plonk_stages(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n,
                           const unsigned lam_key[11], unsigned flags, uint8_t* out, int device);
int bn254_dbg_plonk_stages_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride,
                                const uint8_t* public_inputs, size_t input_stride, size_t n, const unsigned lam_key[11], unsigned flags, uint8_t* out, int device);

/* host-only probe of the GLV scalar decomposition the PlonK MSMs use: k = (-1)^neg1 k1 + (-1)^neg2 k2 lambda (mod r), k1, k2 < 2^127 */
int bn254_dbg_glv_decompose(const uint8_t k32[32], uint8_t k1_16[16], uint8_t k2_16[16], int* neg1, int* neg2);

/* host-only probes of the PlonK batch plan (sub-batches side by side, proofs per sub-batch, proofs per pass) and of the MSM launches (csrc/bn254_msm.h): the row plan of
 * the stage-1 / stage-2 launch for a key with n_qcp commitments and n proofs under a lane budget (0 = the library's) -- rows, rows that use window-table scratch, the
 * scratch lanes that launch needs, its longest row in the planner's cost units, rows and fixed terms per sum, optionally the rows themselves (MSM_MAX_ROWS = 32 rows x 9 ints:
 * variable term (-1: none, or a joint row), pos_lo, pos_hi, unit term, sum, first scratch slot, fixed windows [lo, hi), and for a JOINT row -- several variable terms
 * walked together over all 128 positions, large launches -- the bit mask of its terms); and the scratch lanes a context of `capacity` proofs allocates for launches
 * of n_var variable terms.  tests/test_capi_cpu.py: need <= allocation for every n <= capacity. */
int bn254_dbg_plonk_plan(size_t n, size_t piece, int max_workers, int* workers, size_t* per_worker, size_t* per_pass);
/* host-only probe of the Groth16 plan (csrc/bn254_g16_plan.h: the functions the library itself allocates and enqueues by): a key with key_inputs public inputs
 * (comb != 0: comb tables), a context reserved for `reserved` proofs, a batch of n proofs with n_public inputs each.  alloc = {workspace bytes, partial-sum bytes,
 * digit bytes, proofs per launch of the wide MSM}; out: 8 values per launch {chunk, first proof in the chunk, proofs, stream slot (-1 = the caller's stream),
 * form (0 lane kernels, 1 cooperative, 2 latency mode), Miller steps per launch, first workspace byte, one past its last}.  tests/test_capi_cpu.py walks batch
 * sizes against reservations: every launch inside the allocation, concurrent launches disjoint, the batch covered exactly once. */
int bn254_dbg_g16_plan(size_t key_inputs, int comb, size_t reserved, size_t n, size_t n_public, int n_streams, int single_stream, uint64_t alloc[4], uint64_t* out,
                       int max_launches, int* n_launches);
/* ... and of the compaction of its lane launches (csrc/bn254_g16_plan.h::g16_compacts, g16_compact_alloc): the same walk for a call with `flags`.  alloc = {slot -> proof
 * bytes, slot status bytes, block count bytes} the context holds beside its workspace; out: 6 values per launch {compacts (0 / 1), first slot, slots, first block
 * count, block counts, form} -- a launch that compacts addresses slots [first, first + slots rounded up to 256) and that many / 256 block counts. */
int bn254_dbg_g16_compact_plan(size_t key_inputs, size_t reserved, size_t n, size_t n_public, unsigned flags, int n_streams, int single_stream, uint64_t alloc[3],
                               uint64_t* out, int max_launches, int* n_launches);
/* the launch knobs of the environment as this process read them, once (csrc/bn254_g16_plan.h::launch_knobs; host only, no device): out = {1 unless BN254_COOP=0;
 * what BN254_MILLER_RUN_STEPS means to the four launchers that read it -- steps per launch of a Groth16 batch under one key and over a key list (-1: the plan's
 * choice; 0, one key only: one launch per step), of PlonK's two-pair check under one key (0: one launch per operation) and over a key list; BN254_COOP_FIXED_MAX, the
 * largest two-pair check that takes the cooperative kernel, clamped to an int} */
int bn254_dbg_launch_knobs(int out[6]);
/* host restatement of the count -> scan -> write step of a launch that compacts (k_g16_classify's counts, k_g16_compact_write; the scan through the function the kernel
 * runs): pending = n bytes (non-zero: the proof is still pending after the loader's final checks); slot_proof_out / slot_status_out receive n entries each,
 * *n_pending_out the length of the dense list */
int bn254_dbg_g16_compact(const uint8_t* pending, size_t n, unsigned* slot_proof_out, uint8_t* slot_status_out, unsigned* n_pending_out);
/* ... and of BN254_FLAG_RLC's group status bytes: what the launch parts of a chunk of m proofs address (need) against what a context whose RLC buffers were sized
 * for `reserved` proofs holds (alloc) */
int bn254_dbg_g16_rlc_plan(size_t reserved, size_t m, int n_streams, int log2_group, int log2_share, size_t min_lanes, uint64_t* need, uint64_t* alloc);
/* ... and of its wide form (keys with more than 8 public inputs, csrc/bn254_g16_plan.h::g16_rlc_wide_alloc): alloc = {group scalar row bytes, digit bytes, partial-sum bytes}
 * a context allocates for a chunk of m proofs against a key of key_inputs inputs whose tables have msm_form (0 comb, 1 byte windows, 2 13-bit windows); parts_out: 2 values
 * per launch part {first group, groups}, as the enqueue places them (at most max_parts written, *n_parts = parts) */
int bn254_dbg_g16_rlc_wide_plan(size_t m, int n_streams, int log2_group, int log2_share, size_t min_lanes, size_t key_inputs, int msm_form, uint64_t alloc[3],
                                uint64_t* parts_out, int max_parts, int* n_parts);
/* ... and the groups themselves, under the knobs as this process holds them (BN254_RLC_GROUP_LOG2, BN254_RLC_SHARE_LOG2, BN254_STREAMS, share_min_lanes of
 * bn254_set_rlc_params) -- the plan the enqueue makes for a chunk of m proofs (at most 1 048 576), host only: out_group[i] = the group of proof i, numbered through the
 * chunk (the groups of the launch parts before its own come first); out_log2_share[i] = log2 of the proofs per Miller-loop lane in its launch part */
int bn254_dbg_g16_rlc_groups(size_t m, unsigned* out_group, uint8_t* out_log2_share);
/* the decision of bn254_groth16_stream_overlap replayed over n_batches batches of one (key, device), host only (csrc/bn254_overlap_vote.h: the functions the enqueue
 * itself calls, in its order -- read the measurement an earlier batch recorded, begin the batch, measure it if the question is open).  kind[b]: 0 the batch cannot be
 * measured (it would not run two sub-batches of nearly equal size side by side); 1 it can, and its events will read timings[4 b ..] = {a0, a1, s1, e1} ms: the durations
 * of part 0 and part 1, start and end of part 1 after the start of part 0 (overlap = (a0 + a1) / their union); 2 it can, but its timings cannot be had.  fallback:
 * BN254_STREAM_FALLBACK (0 reports only).  out[4 b ..] = {1: the batch is a re-probe, the single_stream its chunks are planned with, state after the batch (0 open,
 * 1 this batch is being measured, 2 settled), "one after the other" readings in a row}; ratio_out[b] = the last overlap read (-1: none yet) */
int bn254_dbg_overlap_replay(const uint8_t* kind, const float* timings, size_t n_batches, int fallback, int* out, float* ratio_out);
/* host compile of k_g16_decompress's body (csrc/bn254_codec.h::g16_decompress_record) over k compressed records at `stride` (>= 128): raw_out receives k raw 256-byte
 * records, pre_out k bytes (0: decompressed, 1: one of the three points did not decompress -- its raw record is then all ones) */
int bn254_dbg_g16_decompress(const uint8_t* records, size_t stride, size_t k, uint8_t* raw_out, uint8_t* pre_out);
/* the body of k_sp1_public_inputs (csrc/bn254_sha256.h) over n proofs, with the device entries' range rule (pv_bytes): rows_out receives n rows vkey_hash | digest
 * (64 bytes each), bad_out n bytes (1: the range is not inside [0, pv_bytes) -- the row then holds the digest of the empty string).  device -1: compiled for
 * the host; device >= 0: the kernel on that device */
int bn254_dbg_sp1_public_inputs(const uint8_t* vkey_hashes, size_t vkey_stride, const uint8_t* public_values, size_t pv_bytes, const uint64_t* pv_offsets, size_t n,
                                uint8_t* rows_out, uint8_t* bad_out, int device);
/* the row scratch an SP1 Groth16 batch of n proofs needs (csrc/bn254_g16_plan.h::g16_sp1_alloc): out = {proofs it holds, bytes of rows (the pre bytes start there),
 * bytes of pre-status bytes} */
int bn254_dbg_g16_sp1_alloc(size_t n, uint64_t out[3]);
/* host compile of the wide RLC group stage (csrc/bn254_rlc.h: rlc_group_scalar, vm_rlc_group_points_wide) on given data: n proofs in the groups of
 * rlc_plan(n, log2_group, log2_share), weights (16 bytes per proof: k1, k2 as little-endian u64, r_i = k1 + k2 lambda mod r), live (n bytes, 0: the proof
 * contributes weight 0), inputs (n x n_public x 32 bytes, big-endian, used modulo r); kpts = K_0 .. K_n_public and alpha64, uncompressed.  *groups_out = groups;
 * scalars_out = nullptr stops there, else it receives every group's scalars s_gj = sum_i r_i x_ij mod r (groups x n_public x 32 bytes, big-endian) and l_out the
 * point t_0 K_0 + sum_j s_gj K_j of group `group` (t_0 = sum of its live weights), uncompressed, all zero for the identity */
int bn254_dbg_rlc_wide_group(const uint8_t* kpts, const uint8_t alpha64[64], const uint8_t* weights, const uint8_t* live, const uint8_t* inputs, size_t n_public, size_t n,
                             int log2_group, int log2_share, unsigned group, uint8_t* scalars_out, unsigned* groups_out, uint8_t l_out[64]);
size_t bn254_dbg_plonk_scratch_lanes(size_t capacity, int n_var);
/* ... and the projective points (rows x items) the row buffer of a context of `capacity` proofs holds for launches of that key shape and stage (stage 3: the weighted
 * second launch of BN254_FLAG_RLC): n_rows x n of every launch over n <= capacity items must fit (tests/test_msm_rows.py) */
size_t bn254_dbg_plonk_part_points(size_t capacity, int n_qcp, int stage);
int bn254_dbg_plonk_msm_plan(int n_qcp, int stage, size_t n, size_t lane_budget, int* n_rows, int* n_var_rows, size_t* scratch_lanes, int* chain, int sum_rows[2],
                             int fixed_terms[2], int* rows_out);

/* host-only probe of the modular inversion of the PlonK stages (which = 0: the constant-time form the stages use, 1: the Fermat form, 2: the classic
 * shift-and-subtract binary GCD; field 0: Fr, 1: Fp); 32-byte big-endian in / out */
int bn254_dbg_fr_inverse(const uint8_t in32[32], uint8_t out32[32], int which, int field);
/* host-only probe of the two Montgomery product forms of the PlonK stages (form 32: 8 x 32-bit words, what the device runs; 64: 4 x 64-bit limbs, what the host
 * runs): n products of 32-byte big-endian values (reduced first), out = canonical big-endian a * b mod m (field 0: Fr, 1: Fp) */
int bn254_dbg_fr_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int form, int field);

/* host-only probe of the comb tables used for keys with many public inputs (csrc/bn254_host.hpp::build_comb_table): x * P computed from P's table
 * and the column digits of the 256-bit big-endian x, as the kernels do; out64 = uncompressed point, all zero for the identity */
int bn254_dbg_comb_mul(const uint8_t p64[64], const uint8_t x32[32], uint8_t out64[64]);
/* prepared keys the single-proof entries keep (BN254_KEY_CACHE in the environment: unset 4, 0 off, N up to 64) */
int bn254_dbg_key_cache_slots(void);
/* the fixed-base tables `device` built for a key (csrc/bn254_k_comb.hip) against host arithmetic, as field values; *mismatches = entries that differ.  Comb tables (more
 * than 16 public inputs): every entry of the first `inputs` inputs against bn254_host.hpp::build_comb_table.  13-bit window tables (up to 16 inputs): every window's first,
 * middle and last entries and a pseudo-random sample of every input, each against d 2^(13 w) K by double-and-add. */
int bn254_dbg_comb_table_compare(const bn254_g16_pvk* pvk, int device, int inputs, size_t* mismatches);
/* the grouping of a batch over many keys (csrc/bn254_keys.h): slot -> proof index (all ones: a padding slot) and granule (64 slots) -> key.  out_slot_to_proof holds
 * bn254_dbg_g16_keys_slot_bound(n, n_keys) words, out_granule_key a word per 64 of them; *out_n_slots: slots in use.  device -1: compiled for the host; >= 0: the
 * kernels on that device */
size_t bn254_dbg_g16_keys_slot_bound(size_t n, size_t n_keys);
int bn254_dbg_g16_keys_group(const unsigned* key_index, size_t n, size_t n_keys, int device, unsigned* out_slot_to_proof, unsigned* out_granule_key, size_t* out_n_slots);
/* the plan of a batch of n proofs over n_keys keys (csrc/bn254_g16_plan.h, the function the entries enqueue by; host only).  *form: 0 grouped lanes, 1 direct
 * cooperative; *slots: n, or bn254_dbg_g16_keys_slot_bound(n, n_keys); *launches: kernels + memsets a raw-record batch enqueues through the device entry (without the
 * kernel of BN254_FLAG_STRICT_SCALARS) */
int bn254_dbg_g16_keys_plan(size_t n, size_t n_keys, int* form, size_t* slots, int* launches);
/* the form of the last batch enqueued on the cached state of (list, device): 0 or 1 as above, -1 if there was none (also: the list is not cached) */
int bn254_dbg_g16_keys_last_form(const bn254_g16_pvk* const* pvks, size_t n_keys, int device, int* form);
/* The plan of a PlonK batch over many keys (host arithmetic only): n proofs over n_keys entries whose grouping came to `slots` slots (a multiple of 64), under the
 * current knobs.  slot_bound: n + min(n_keys, n) * 63 rounded to 64; workers / per_worker / per_pass: sub-batches side by side, slots per sub-batch, slots per pass;
 * ctx_capacity: slots a context holds after bn254_plonk_reserve_keys for (n, n_keys); pass_first: the first slot of each pass (up to cap entries), n_passes: how many. */
int bn254_dbg_plonk_keys_plan(size_t n, size_t n_keys, size_t slots, size_t* slot_bound, int* workers, size_t* per_worker, size_t* per_pass, size_t* ctx_capacity,
                              size_t* pass_first, size_t cap, size_t* n_passes);
/* k_coop12_miller_fixed_keys, the cooperative two-pair check with the key per item, in store mode on the line tables of prepared PlonK keys (shaped as
 * bn254_dbg_coop12_miller_fixed; the members are made ready on the device first): item i belongs to pvks[key_words[i >> key_shift]] (a word >= n_keys reads key 0),
 * g1_0 / g1_1: n affine G1 points of 64 bytes each, identity: null or per item bit 0 / bit 1 = pair 0 / pair 1 is the identity, out_gt: 384 bytes per item, the
 * final-exponentiated e(P0, Q0_k) e(P1, Q1_k) with the two KZG G2 points of the item's key.  n at most 40 960. */
int bn254_dbg_coop12_miller_fixed_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_words, unsigned key_shift, const uint8_t* g1_0,
                                       const uint8_t* g1_1, const uint8_t* identity, uint8_t* out_gt, size_t n, int device);
/* the knobs of a PlonK batch over a key list as they are now: out[0] coop_max (bn254_set_plonk_keys_params), out[1] min_pass (bn254_set_plonk_rlc_params) */
int bn254_dbg_plonk_keys_knobs(long out[2]);
/* the host image of a prepared Groth16 key, serialised: dwords n_k (2) | msm_comb | k0, gtab, dtab, target, kpts, each as its length and its dwords | alpha (18),
 * k0_pt (18), b_arg (36) as canonical digits.  Two handles of one key are interchangeable iff their images are equal.  *len: bytes of the image (always written);
 * a null or too small out (cap bytes) is BN254_E_BAD_ARG */
int bn254_dbg_g16_pvk_image(const bn254_g16_pvk* pvk, uint8_t* out, size_t cap, size_t* len);
/* bn254_groth16_vk_prepare_batch with a choice of where the bodies of its kernels run (csrc/bn254_vkprep.h): device -1 is their host compile -- no device is touched,
 * e(alpha, beta) by the host's Miller loop -- a device ordinal the kernels.  stage_ms: null, or 5 floats: G1 decode, G2 decode, fold, line tables, pairing program,
 * summed over the passes, from HIP events (zero on the host) */
int bn254_dbg_g16_vk_prepare_batch(const uint8_t* const* vks, const size_t* vk_lens, size_t n_keys, unsigned mode, int device, bn254_g16_pvk** out, int* key_status,
                                   float* stage_ms);
int bn254_dbg_plonk_table_compare(const bn254_plonk_pvk* pvk, int device, size_t* mismatches);   /* the window tables of a PlonK key's points (csrc/bn254_fw.h): every window's first, middle and last entries and a pseudo-random sample */

/* Revision of this header's binary interface: bumped whenever a function changes its arguments, an array argument its length or a slot its meaning (5:
 * BN254_PLONK_NUM_TIMINGS has been 9 since revision 4, bn254_dbg_plonk_msm_plan writes 9 ints per row).  Entries that are only ADDED -- the batches over many
 * keys, bn254_set_keys_params, bn254_groth16_vk_prepare_batch, bn254_set_pairing_params / bn254_pairing_params / bn254_pairing_state, bn254_g2_prepare and the bn254_pairing_*_shared entries, the bn254_kzg_* entries, bn254_kzg_verify_folded_batch / _device / bn254_kzg_fold_reserve, bn254_pairing_check_batch_flags / _device, bn254_set_pairing_rlc_params / bn254_pairing_rlc_params / bn254_pairing_rlc_state and their probes -- change no existing function, array or slot, so the revision stays: a binding that needs them finds out when it resolves their symbols.  A binding compares it with the value it was generated for. */
#define BN254_ABI_VERSION 5
int bn254_abi_version(void);
const char* bn254_status_string(int status_byte);
const char* bn254_last_error(void);
const char* bn254_version(void);

#ifdef __cplusplus
}
#endif
#endif
