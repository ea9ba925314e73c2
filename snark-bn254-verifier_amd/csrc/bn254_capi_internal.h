// bn254_capi_internal.h -- what the translation units of the C ABI (bn254_capi*.hip) share: the per (key, device) state of both protocols, the key
// cache of the single-proof entries, and the helpers more than one of them calls.  Private: nothing outside csrc/ includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <dlfcn.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/bn254_verify.h"
#include "bn254_host.hpp"
#include "bn254_plonk.hpp"
#include "bn254_rlc.h"
#include "bn254_g16_plan.h"
#include "bn254_overlap_vote.h"
#include "bn254_keys.h"
#include <sys/random.h>
#include <atomic>
#include <thread>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <chrono>
#include <cstdio>
#include <stdexcept>

using namespace bn254host;

// bn254_k_plonk.hip: the PlonK host stages as device kernels (the same bn254_plonk.hpp source, one proof per lane)
size_t bn254_plonk_work_bytes();
size_t bn254_plonk_key_bytes();
hipError_t bn254_plonk_dev_init(int device);
hipError_t bn254_plonk_self_test(const void* key_host, const void* d_key, std::string* why);
hipError_t bn254_launch_plonk_stage1(const void* d_key, const uint8_t* d_proofs, size_t stride, const uint8_t* d_inputs, size_t n_public, size_t n, const uint32_t lam_key[11],
                                     void* d_work, void* d_terms, uint8_t* d_flags, int T1, hipStream_t s);
hipError_t bn254_launch_plonk_stage2(const void* d_key, const uint8_t* d_proofs, size_t stride, size_t n, void* d_work, const uint32_t* d_lin_words, const uint8_t* d_lin_inf,
                                     void* d_terms, uint8_t* d_flags, uint8_t* d_status, int TT, int T2, const uint32_t* weight_key, hipStream_t s);
// the stages over the slots of a batch over many keys (bn254_keys.h: the key per granule of 64 slots)
hipError_t bn254_launch_plonk_stage1_keys(const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const uint8_t* d_recs, size_t rec_stride, size_t proof_len,
                                          const uint8_t* d_inputs, size_t in_stride, size_t staged_public, size_t n, const uint32_t lam_key[11], void* d_work, void* d_terms,
                                          uint8_t* d_flags, int T1, hipStream_t s);
// weight_key != nullptr: BN254_FLAG_RLC, the weight stream of bn254_launch_plonk_stage2
hipError_t bn254_launch_plonk_stage2_keys(const bn254::PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const uint8_t* d_recs, size_t rec_stride, size_t n,
                                          void* d_work, const uint32_t* d_lin_words, const uint8_t* d_lin_inf, void* d_terms, uint8_t* d_flags, uint8_t* d_status, int TT, int T2,
                                          const uint32_t* weight_key, hipStream_t s);
hipError_t bn254_launch_plonk_group_sums(int32_t* ws, const uint8_t* status, size_t n, int32_t* grp_ws, uint8_t* grp_status, int e_p0, int inf0, int e_p1, int inf1, hipStream_t s);
hipError_t bn254_launch_plonk_group_scatter(uint8_t* status, size_t n, const uint8_t* grp_status, uint32_t* n_failed, hipStream_t s);

hipError_t bn254_launch_plonk_dbg_zeta(const void* d_work, size_t n, uint8_t* d_zeta, uint8_t* d_status, hipStream_t s);
// the values the stages left for n proofs (slots), PLONK_DBG_STAGES_DEV_BYTES per proof (k_plonk_dbg_stages has the layout; n_h2f: hash-to-field values per proof, at most 8)
#define PLONK_DBG_STAGES_DEV_BYTES 432
hipError_t bn254_launch_plonk_dbg_stages(const void* d_work, const uint32_t* d_lin_words, const uint8_t* d_lin_inf, const uint8_t* d_status, size_t n, uint32_t n_h2f, uint8_t* d_out,
                                         hipStream_t s);

#pragma GCC visibility push(hidden)
extern thread_local std::string g_err;     // bn254_last_error() of the calling thread
int set_err(int code, const std::string& msg);
#pragma GCC visibility pop
#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return set_err(BN254_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#include "bn254_capi_owners.h"

// Initial values of the knobs come from the environment, read ONCE when the library is loaded (getenv racing a host's setenv is undefined behaviour).
static inline long env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }

// BN254_FLAG_RLC: per (key, device) buffers of the random-linear-combination batch mode (bn254_rlc.h)
struct RlcDev {
  bool ready = false;
  DevBuf<int32_t> btab, tab, one;                                     // key-side tables (uploaded once)
  // group status bytes and the indices of the pending proofs with their pinned copies: sized together for grp_cap proofs (rlc_ensure)
  DevBuf<uint8_t> grp_status; DevBuf<uint32_t> idx; PinBuf<uint8_t> h_status; PinBuf<uint32_t> h_idx; size_t grp_cap = 0;
  // the exact second pass: records, input rows and status bytes of the proofs of failed groups, for fb_cap proofs (grown by the pass that needs more)
  DevBuf<uint8_t> fb_proofs, fb_inputs, fb_status; size_t fb_cap = 0, fb_in_cap = 0;
  // keys with more than RLC_MAX_PUBLIC inputs: group scalar rows, digits and chunk sums of the groups' MSM (bn254_g16_plan.h::g16_rlc_wide_alloc), for wide_cap groups
  DevBuf<uint8_t> grp_rows; DevBuf<uint16_t> grp_digits; DevBuf<int32_t> grp_part; size_t wide_cap = 0;
  // adaptive use of the mode: share of the checked proofs the last RLC passes sent to the exact fallback (exponential average) and how many
  // calls have bypassed the mode since the last pass that measured it
  bool have_obs = false; float fb_share = 0.f; unsigned bypassed = 0, bypassed_total = 0;
};

// per-launch timing of one sub-batch: `own` owns the events, `ev` is the array the launcher records into (prof.ev), `kid` the kind of each pair (prof.kid)
struct G16ProfPool { std::vector<Event> own; std::vector<hipEvent_t> ev; std::vector<uint8_t> kid; G16Prof prof{0, nullptr, nullptr, 0, 0}; };

// Per (key, device) state.  `mu` serialises everything that touches it: uploads, (re)allocation and the enqueue of a batch.  The
// workspace and the staging buffers are shared by all batches against this key on this device, so a batch first waits (on the GPU:
// hipStreamWaitEvent) for `busy_ev`, the completion event of the previous batch, whatever stream that one ran on.
struct DevState {
  std::mutex mu;
  bool ready = false;
  DevBuf<int32_t> k0, gtab, dtab, target, msm;
  DevBuf<int32_t> ws;                                               // G16_WS_BYTES_PER_PROOF per proof
  size_t ws_proofs() const { return ws.cap() / (size_t)(G16_WS_BYTES_PER_PROOF / 4); }
  DevBuf<int32_t> msm_part; size_t msm_part_cap = 0, msm_chunks = 0;                // wide keys: partial sums of the public-input MSM (proofs it holds)
  // launches that compact (bn254_g16_plan.h::g16_compacts): slot_proof | block counts | slot_status for compact_cap proofs, sized with the workspace by ensure_dev
  // (g16_compact_alloc); 0 for a key whose launches never compact
  DevBuf<uint32_t> compact; size_t compact_cap = 0;
  DevBuf<uint8_t> st_proofs, st_inputs, st_status;                  // staging for the host-buffer entry point, through `ring`
  PinRing ring;                                                     // host-buffer entry: copy / compute overlap
  Event busy_ev; bool busy_valid = false;
  Event ev[5]; bool ev_ready = false; bool ev_recorded = false;
  // concurrent sub-batches (see g16_enqueue_exact): part 0 runs on the caller's stream, parts 1..3 on these, created when first needed -- every
  // stream of a process shares the runtime's few hardware queues (four by default), and a copy stream that lands on the queue of a busy compute
  // stream waits behind its kernels (measured: 3 GB/s instead of 55), so no stream is created that is not used
  Stream aux[3]; Event fork_ev, join_ev[4];
  // per-launch timing of the first sub-batch (pool 0: bn254_groth16_kernel_profile) and of the SECOND, whose launches run on another stream beside the first's
  // (pool 1, when prof2_used: bn254_groth16_kernel_profile_all)
  G16ProfPool prof[2]; bool prof2_used = false; size_t prof_n = 0; unsigned prof_epoch = 0;
  RlcDev rlc;                                                       // BN254_FLAG_RLC buffers (bn254_rlc.hpp)
  // BN254_FLAG_COMPRESSED_PROOFS: raw records of the decompressed chunk, then one pre-status byte per proof (bn254_g16_plan.h::g16_cmp_alloc); grown at the
  // first compressed batch that needs more
  DevBuf<uint8_t> cmp;
  size_t cmp_proofs() const { return cmp.cap() / 257; }
  // SP1 public inputs: rows vkey_hash | digest of the hashed chunk, then one pre-status byte per proof (bn254_g16_plan.h::g16_sp1_alloc), grown at
  // the first SP1 batch that needs more.  The host-buffer entry stages the batch's values, offsets and vkey hashes in st_pv / st_off / st_vkh.
  DevBuf<uint8_t> sp1;
  size_t sp1_proofs() const { return sp1.cap() / 65; }
  DevBuf<uint8_t> st_pv, st_off, st_vkh;
  // do the sub-batch streams overlap?  ov_ev: start / end of part 0 and of part 1 of a measured two-stream batch; ov: what was read from them and what follows
  // from it (bn254_overlap_vote.h)
  Event ov_ev[4]; OvVote ov;
};
struct bn254_g16_pvk {
  G16Prepared host;
  mutable G16PreparedRlc rlc_host;       // built on the first BN254_FLAG_RLC batch (under mu)
  mutable std::mutex mu;                 // protects the map below (lookup / insertion only) and rlc_host
  mutable std::map<int, DevState> dev;
};

// ---------------------------------------------------------------- PlonK (BASELINE configs[3])
// One PlonkCtx = one sub-batch in flight: its own stream, device buffers and pinned host staging.  A batch is cut into sub-batches that worker
// threads drive concurrently, so the host work of one sub-batch (staging copies, status read-back) overlaps the GPU stages of the others; every
// wait is stream-scoped.
#define PLONK_WORKERS 8
// proofs per pass at most.  Until round 4 this was 65 536 -- one wavefront per SIMD for every one-lane-per-proof kernel of a pass, which left the pairing stage of the
// largest passes at 0.39 of the multiply-add peak; a pass of 2^18 proofs gives the same kernels four (the context's buffers for it: 5.4 GB at the SP1 key shape)
#define PLONK_MAX_LAUNCH 262144
struct PlonkCtx {
  size_t cap = 0;                      // proofs the buffers below hold
  Stream stream, aux; Event ev_fork, ev_join;
  Event tk[8];   // timing: before stage 1 | after it | MSM rows | sum | stage 2 | MSM rows | sums | pairing check
  float last_ms[BN254_PLONK_NUM_TIMINGS] = {0}; size_t last_lanes[2] = {0, 0}; bool last_valid = false;
  DevBuf<int32_t> ws, part, glv_tab;   // part: the rows of an MSM launch (bn254_msm.h); glv_tab: the window tables of its variable rows
  size_t part_points = 0;              // projective points (rows x items) `part` holds (plonk_part_points of the capacity)
  size_t glv_lanes = 0;                // lanes glv_tab holds (plonk_scratch_lanes of the capacity); a launch checks its need against it before it is enqueued
  DevBuf<MsmTerm> terms; DevBuf<uint8_t> flags; DevBuf<uint32_t> words; DevBuf<uint8_t> inf, status;
  PinBuf<uint8_t> h_status;            // pinned: the status bytes of a pass on their way back
  // device-side stages (bn254_k_plonk.hip): the batch's proofs and inputs in device memory (through a pinned copy: both of in_cap() bytes, or neither), per-proof state between the stages
  DevBuf<uint8_t> d_in; PinBuf<uint8_t> h_in; DevBuf<uint8_t> d_work;
  size_t in_cap() const { return h_in.cap(); }
  // BN254_FLAG_RLC: the pairing checks of a pass batched over groups of 64 proofs -- the groups' points and status bytes in a workspace of their own, failed groups counted
  DevBuf<int32_t> grp_ws; DevBuf<uint8_t> grp_status; DevBuf<uint32_t> d_fail; PinBuf<uint32_t> h_fail;
};
struct PlonkDev {
  bool ready = false;
  DevBuf<int32_t> tab0, tab1, one;
  DevBuf<int32_t> fixed_tabs;          // window tables of the key's G1 points (plonk_num_tables x MSM_FW_WINDOWS x MSM_FW_ENTRIES entries, bn254_fw.h)
  DevBuf<uint8_t> d_key;               // the parsed key (PlonkKey) for the device-side stages
  PlonkCtx ctx[PLONK_WORKERS];
  // The contexts are handed out to calls: a call takes one per sub-batch (all at once, so two calls cannot wait for each other) and returns them when it
  // is done.  Calls on ONE prepared key from several host threads therefore run side by side, up to PLONK_WORKERS sub-batches in flight; at 4096 proofs a
  // batch is a chain of latency-bound launches that leaves most of the GPU idle, and two batches in flight verify 1.35 x as many proofs per second.
  std::mutex pool_mu; std::condition_variable pool_cv; bool busy[PLONK_WORKERS] = {};
  float last_ms[BN254_PLONK_NUM_TIMINGS] = {0}; size_t last_lanes[2] = {0, 0}; bool last_valid = false;   // first sub-batch of the call that finished last
  // SP1 entries (bn254_capi_sp1.hip): device buffers for the rows, pre-status bytes and staged values of a call.  A call takes one for itself (calls on one key run side
  // by side, so the rows cannot live in the key's state) and gives it back for the next call: a hipFree per call would wait for every other call's work on the device
  std::mutex sp1_mu; std::vector<DevBuf<uint8_t>> sp1_bufs;
};
struct PlonkLease {   // the contexts of one call
  PlonkDev* d; int idx[PLONK_WORKERS]; int n = 0;
  PlonkLease(PlonkDev* d_, int want) : d(d_) {
    std::unique_lock<std::mutex> lk(d->pool_mu);
    d->pool_cv.wait(lk, [&] { int f = 0; for (bool b : d->busy) f += b ? 0 : 1; return f >= want; });
    for (int i = 0; i < PLONK_WORKERS && n < want; i++) if (!d->busy[i]) { d->busy[i] = true; idx[n++] = i; }
  }
  PlonkCtx& ctx(int w) const { return d->ctx[idx[w]]; }
  ~PlonkLease() {
    {
      std::lock_guard<std::mutex> lk(d->pool_mu);
      const PlonkCtx& c = d->ctx[idx[0]];
      if (c.last_valid) { for (int i = 0; i < BN254_PLONK_NUM_TIMINGS; i++) d->last_ms[i] = c.last_ms[i]; d->last_lanes[0] = c.last_lanes[0]; d->last_lanes[1] = c.last_lanes[1]; d->last_valid = true; }
      for (int i = 0; i < n; i++) d->busy[idx[i]] = false;
    }
    d->pool_cv.notify_all();
  }
  PlonkLease(const PlonkLease&) = delete; PlonkLease& operator=(const PlonkLease&) = delete;
};
struct bn254_plonk_pvk {
  PlonkKey key;
  std::vector<int32_t> tab0, tab1, one;
  std::vector<int32_t> fixed_pts;      // every key point that enters an MSM (bn254_plonk.hpp::plonk_table_point) as affine digits, 18 dwords each: their window tables
                                       // (MSM_FW_BITS, bn254_fw.h) are built on the device that uses them (bn254_k_comb.hip form 2)
  MsmShape shape1, shape2, shape2_rlc; // term kinds of the two MSM launches (plonk_msm1_shape / plonk_msm2_shape; _rlc: the weighted form of BN254_FLAG_RLC)
  mutable std::mutex mu;               // protects the map below (lookup / insertion / first upload); batches take contexts from the device's pool
  mutable std::map<int, PlonkDev> dev;
};

// ---- prepared keys of the single-proof entry points (bn254_groth16_verify, bn254_plonk_verify): the last KEY_CACHE_SLOTS keys by exact bytes.
// Entries are shared_ptrs: an evicted key is freed when its last in-flight call returns.  The cache object itself is never destroyed (keys hold
// device memory; freeing it from a static destructor would race the HIP runtime's own teardown).  BN254_KEY_CACHE=0 switches it off, BN254_KEY_CACHE=N (1 .. 64) sets the
// number of keys kept (a caller that rotates through more keys than slots pays the preparation, ~9 ms of an 11 ms call, on every miss).
#define KEY_CACHE_SLOTS 4
#define KEY_CACHE_MAX_SLOTS 64
template <class T, void (*FREE)(T*)>
class KeyCache {
 public:
  std::shared_ptr<T> find(const uint8_t* vk, size_t len, unsigned mode) {
    if (!slots()) return nullptr;
    std::lock_guard<std::mutex> lk(mu_);
    for (auto& e : e_)
      if (e.h && e.mode == mode && e.bytes.size() == len && memcmp(e.bytes.data(), vk, len) == 0) { e.tick = ++clock_; return e.h; }
    return nullptr;
  }
  static int capacity() { return slots(); }
  std::shared_ptr<T> insert(const uint8_t* vk, size_t len, unsigned mode, T* raw) {
    std::shared_ptr<T> h(raw, [](T* p) { FREE(p); });
    if (!slots()) return h;
    std::lock_guard<std::mutex> lk(mu_);
    Entry* v = &e_[0];
    for (auto& e : e_) { if (!e.h) { v = &e; break; } if (e.tick < v->tick) v = &e; }
    v->bytes.assign(vk, vk + len); v->mode = mode; v->h = h; v->tick = ++clock_;
    return h;
  }

 private:
  // unset: KEY_CACHE_SLOTS; 0: off; N: N slots (at most KEY_CACHE_MAX_SLOTS)
  static int slots() { static const int n = [] { const char* e = getenv("BN254_KEY_CACHE"); long v = e ? atol(e) : KEY_CACHE_SLOTS; return (int)(v < 0 ? 0 : (v > KEY_CACHE_MAX_SLOTS ? KEY_CACHE_MAX_SLOTS : v)); }(); return n; }
  struct Entry { std::vector<uint8_t> bytes; unsigned mode = 0; std::shared_ptr<T> h; uint64_t tick = 0; };
  std::mutex mu_; std::vector<Entry> e_ = std::vector<Entry>((size_t)(slots() > 0 ? slots() : 1)); uint64_t clock_ = 0;
};

// ---- key sets of the batches over many keys (bn254_capi_keys.hip, bn254_capi_plonk_keys.hip): the last KEYS_SET_SLOTS (list, device) pairs, least recently used out
// first.  Set has the members `list` (the handles as passed), `device` and `max_public`, which get() fills; everything else of a set is made ready by its first user,
// under the set's own lock.  Entries are shared_ptrs: a set that is evicted, or dropped because one of its members was freed, releases its device memory when the last
// call that still holds it returns.  Never destroyed (as the key cache: device memory must not be freed from a static destructor).
#define KEYS_SET_SLOTS 4
template <class Set, class Handle>
struct KeySetCache {
  std::shared_ptr<Set> get(const Handle* const* pvks, size_t n_keys, int device, size_t max_public) {
    std::shared_ptr<Set> evicted, out;      // evicted: released outside the lock (its destructor waits for the device)
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (Entry* x = lookup(pvks, n_keys, device)) { x->tick = ++clock_; return x->set; }
      Entry* v = &e_[0];
      for (auto& x : e_) { if (!x.set) { v = &x; break; } if (x.tick < v->tick) v = &x; }
      evicted = std::move(v->set);
      out = std::make_shared<Set>();
      out->list.assign(pvks, pvks + n_keys); out->device = device; out->max_public = max_public;
      v->set = out; v->tick = ++clock_;
    }
    return out;
  }
  std::shared_ptr<Set> find(const Handle* const* pvks, size_t n_keys, int device) {      // the cached set of this list, or none: no insertion, no change of the order
    std::lock_guard<std::mutex> lk(mu_);
    Entry* x = lookup(pvks, n_keys, device);
    return x ? x->set : nullptr;
  }
  void drop(const Handle* member) {      // every set that contains the handle; released outside the lock
    std::vector<std::shared_ptr<Set>> gone;
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (auto& x : e_)
        if (x.set && std::find(x.set->list.begin(), x.set->list.end(), member) != x.set->list.end()) gone.push_back(std::move(x.set));
    }
  }

 private:
  struct Entry { std::shared_ptr<Set> set; uint64_t tick = 0; };
  Entry* lookup(const Handle* const* pvks, size_t n_keys, int device) {
    for (auto& x : e_)
      if (x.set && x.set->device == device && x.set->list.size() == n_keys && memcmp(x.set->list.data(), pvks, n_keys * sizeof(*pvks)) == 0) return &x;
    return nullptr;
  }
  std::mutex mu_; Entry e_[KEYS_SET_SLOTS]; uint64_t clock_ = 0;
};

// Shared helpers (internal linkage across the bn254_capi*.hip objects only: none of them is part of the exported ABI)
#pragma GCC visibility push(hidden)
int check_batch_args(bool plonk, const void* pvk, const void* proofs, size_t proof_stride, const void* inputs, size_t n_public, size_t n, const void* status,
                     unsigned flags);
int check_device(int device);
// bn254_capi_selftest.hip: the known-answer self-test of the verdict kernels, once per process and device (include/bn254_verify.h, bn254_device_selftest).  Called after
// check_device by everything that makes a device ready: BN254_OK once the device has passed (or BN254_SELFTEST=0), BN254_E_SELFTEST with the recorded text on one that failed
int selftest_gate(int device);
// a batch over a key list (bn254_capi_keys.hip): the list itself (every handle non-null, at most G16_KEYS_MAX_KEYS entries, no key above G16_KEYS_MAX_PUBLIC inputs; the
// limits are refused with a bn254_last_diagnostic() text) -> *max_public, the largest input count; then the batch arguments against it
int check_key_list(const bn254_g16_pvk* const* pvks, size_t n_keys, size_t* max_public);
int check_keys_args(const bn254_g16_pvk* const* pvks, size_t n_keys, const void* key_index, const void* proofs, size_t proof_stride, const void* inputs, size_t input_stride,
                    size_t n, const void* status, unsigned flags, size_t* max_public);
void set_diag(const std::string& msg);     // bn254_last_diagnostic() of the calling thread (bn254_capi_g16.hip)
void keys_sets_drop(const bn254_g16_pvk* member);   // bn254_capi_keys.hip: forget every cached key set that contains this key
// bn254_capi_keys.hip, for the value probe of the loader over a key list (bn254_dbg_g16_loader_keys, which has checked the arguments and counted the slots): the set
// of the list made ready, the batch grouped, bn254_launch_g16_prepare_keys over all its slots, and what it left read back -- slot_to_proof and the slots' status bytes
// as they are, the twelve elements from VE_AX through `points` (384 stored bytes per slot -> 320).  misalign: the device copy of the rows starts that many bytes
// past a 4-byte boundary
int g16_keys_probe_loader(const bn254_g16_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                          size_t input_stride, size_t n, unsigned flags, int misalign, size_t slots, unsigned* out_slot_proof, uint8_t* out_slot_status, uint8_t* out_points,
                          size_t* out_n_slots, int device, void (*points)(const uint8_t*, size_t, uint8_t*));
void parallel_copy(uint8_t* dst, const uint8_t* src, size_t bytes);
int build_tables_on_device(int form, const std::vector<int32_t>& pts, DevBuf<int32_t>& dst);
int sub_batch_streams();                   // BN254_STREAMS, read once: sub-batches of a Groth16 chunk in flight, 1 .. 4 (default 2)
// bn254_capi_vkbatch.hip: bn254_groth16_vk_prepare_batch and its probe (on_host: the kernels' bodies compiled for the host, no device touched; stage_ms: null or
// the five per-stage times of the device passes)
int vkp_prepare_batch(const uint8_t* const* vks, const size_t* vk_lens, size_t n_keys, unsigned mode, bool on_host, int device, bn254_g16_pvk** out, int* key_status,
                      float* stage_ms);
// bn254_capi_g16.hip
DevState* dev_state(const bn254_g16_pvk* pvk, int device);
int ensure_dev(const bn254_g16_pvk* pvk, DevState& d, int device, size_t n);
// SP1 public inputs (bn254_capi_sp1.hip): where the vkey hashes and the values of a batch are.  Proof i's vkey hash is the 32 bytes at vkh + i vkh_stride
// (vkh_stride 0: one for all), its values the bytes [off[i] - pv_base, off[i+1] - pv_base) of pv, a buffer of pv_bytes bytes; off holds n + 1 entries
struct Sp1Src { const uint8_t* vkh; size_t vkh_stride; const uint8_t* pv; uint64_t pv_bytes, pv_base; const uint64_t* off; };
int check_sp1_args(bool plonk, const void* pvk, const void* proofs, size_t proof_stride, const void* vkh, size_t vkh_stride, const void* pv, uint64_t pv_bytes,
                   const uint64_t* off, bool host_offsets, size_t n, const void* status, unsigned flags);
// the batch on device buffers (enqueued on `user`) / on host buffers (staged through the pinned ring; returns when the status bytes are back)
int g16_sp1_device(const bn254_g16_pvk* pvk, const void* d_proofs, size_t proof_stride, const Sp1Src& s, size_t n, void* d_status, int device, hipStream_t user, unsigned flags);
int g16_sp1_host(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const Sp1Src& s, size_t n, uint8_t* status, int device, unsigned flags);
// bn254_capi_plonk.hip
int plonk_ensure_dev(const bn254_plonk_pvk* pvk, int device, PlonkDev** out);
int plonk_ensure_ctx(const bn254_plonk_pvk* pvk, PlonkCtx& c, size_t n, size_t in_bytes);
int plonk_joint_g(size_t m_pad);
size_t msm_lane_budget();
size_t plonk_scratch_lanes(size_t need, int n_var);
size_t plonk_part_points(size_t need, const MsmShape& shape);
void plonk_plan(size_t n, size_t piece, int max_workers, int* workers, size_t* per, size_t* pass);
void plonk_plan_for(size_t n, int* workers, size_t* per, size_t* pass_cap);     // the plan of a batch of n proofs (or slots) under the current knobs
size_t plonk_piece_for(size_t n, int* max_workers);
int plonk_plan_breaks(size_t out[4]);
size_t plonk_rlc_min();                    // BN254_FLAG_RLC is honoured from this many proofs (slots) per pass (bn254_set_plonk_rlc_params)
// What a pass runs against: ONE key's device state, or (desc != nullptr) the descriptors of a key list with the key of every granule of 64 slots.  The pass driver
// itself never asks which: plonk_msm and the four launch helpers beside it (bn254_capi_plonk.hip) pick the launcher, and launched() the code of a launch that failed
struct PlonkTables {
  const PlonkDev* key; const bn254::PlonkKeyDesc* desc; uint32_t n_keys; const uint32_t* granule_key;
  const int32_t* one;      // 1 in GT, the target of the pairing checks
  int launched(hipError_t e, const char* what) const;
};
// The records and input rows of a pass in device memory, rec_stride bytes from one record to the next.  One key: the caller's own layout, rows of n_public inputs.
// A list: gathered in slot order, proof_len the stride of the caller's records, rows in_stride bytes apart (null: no key has inputs), staged_public as
// bn254_launch_plonk_stage1_keys takes it
struct PlonkPassIn { const uint8_t* recs; size_t rec_stride; const uint8_t* inputs; size_t n_public, proof_len, in_stride, staged_public; };
// what the joint check of a pass did (BN254_FLAG_RLC honoured: ran), and whether the per-proof check ran
struct PlonkPassReport { bool joint = false; size_t groups = 0; uint32_t failed = 0; bool exact = false; };
// one MSM launch of a pass on context c (rows + sums)
int plonk_msm(const PlonkTables& t, PlonkCtx& c, const MsmShape& shape, size_t m, int n_terms, bool to_words, size_t* lanes_out, hipEvent_t ev_rows);
// One pass of m proofs (slots) on context c, from "records and rows are in device memory" to "the status bytes are in c.status", all enqueued on c.stream; shapes: the
// key whose term counts and MSM shapes the pass has.  tk: null, or the eight timing events of PlonkCtx::tk
int plonk_pass(const bn254_plonk_pvk* shapes, const PlonkTables& t, const PlonkPassIn& in, PlonkCtx& c, size_t m, unsigned flags, const Event* tk, PlonkPassReport* rep);
// The first part of that pass under the CALLER's ChaCha20 key: stage 1 -> digest MSM -> stage 2 -> KZG MSM, to the pairing operands at VE_LX / VE_CX of c.ws and the
// status bytes in c.status.  plonk_pass calls it with a key it has just drawn; the only other callers are the value probes of bn254_capi_dbg.hip
int plonk_pass_points(const bn254_plonk_pvk* shapes, const PlonkTables& t, const PlonkPassIn& in, PlonkCtx& c, size_t m, const uint32_t lam_key[11], bool weighted, const Event* tk);
// bn254_capi_plonk_keys.hip, for the value probe over a key list: the arguments of bn254_plonk_verify_batch_keys checked, the batch grouped, and ALL its slots gathered
// as one pass on a leased context (pk_run_pass's front).  body sees what that pass would hand to plonk_pass; slot_to_proof: the slots' proof indices, on the device
struct PlonkKeysProbePass { const bn254_plonk_pvk* shapes; PlonkTables t; PlonkPassIn in; PlonkCtx* c; size_t slots; const uint32_t* slot_to_proof; };
int plonk_keys_probe_pass(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                          size_t input_stride, size_t n, unsigned flags, int device, const std::function<int(const PlonkKeysProbePass&)>& body);
// The passes of a plan -- worker w has items [w per, (w + 1) per) of `total`, `pass` at a time -- on the contexts of a lease: run_pass(w, first, m) inline for one
// worker, on one host thread each otherwise.  The first failure is the call's (set_err)
int plonk_run_workers(const PlonkLease& lease, int workers, size_t per, size_t pass, size_t total, const std::function<int(int, size_t, size_t)>& run_pass);
void plonk_keys_sets_drop(const bn254_plonk_pvk* member);   // bn254_capi_plonk_keys.hip: forget every cached PlonK key set that contains this key
// a PlonK batch whose public inputs are already rows of two inputs in device memory (d_rows, 64 bytes per proof): resident = true, proofs and status are device
// memory too; false, they are host buffers and only the proofs are staged
int plonk_batch_rows(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* d_rows, size_t n, uint8_t* status, int device, unsigned flags,
                     bool resident);
#pragma GCC visibility pop

// dst stays empty unless the copy is complete: a caller that retries after a failure uploads exactly what is still missing (a sanitizer run of the
// allocation-failure paths found the retry overwriting -- leaking -- the tables an earlier, partly failed attempt had already uploaded)
template <typename T> static int upload(DevBuf<T>& dst, const std::vector<T>& src) {
  if (dst) return BN254_OK;
  DevBuf<T> p;
  int rc = p.ensure(src.size());
  if (rc) return rc;
  if (!src.empty()) {
    hipError_t e = hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  dst = std::move(p);
  return BN254_OK;
}

// the table form of a Groth16 key (build_tables_on_device: 0 comb tables, 1 byte windows, 2 windows of MSM_FW_BITS)
static inline int g16_table_form(const G16Prepared& h) { return h.msm_comb ? 0 : h.key_inputs() > (size_t)G16_WIDE_MSM_MIN_INPUTS ? 1 : 2; }
