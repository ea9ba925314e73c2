// bn254_capi_g16.hip -- the Groth16 half of the C ABI (include/bn254_verify.h): per (key, device) state and tables, the exact and RLC enqueue paths,
// the stream-overlap bookkeeping, the pinned ring of the host-buffer entry, and every bn254_groth16_* entry.
#include "bn254_capi_internal.h"

// The HIP runtime multiplexes every stream of the process onto GPU_MAX_HW_QUEUES hardware queues -- four by default -- and streams that share a queue run one
// after the other: the two sub-batch streams of a large Groth16 batch then lose their overlap once a third party (RCCL) has streams too, and eight PlonK chains
// run at 1.20 instead of 1.51 M proofs/s (profiles/r03_batch_sweep_fine.txt).  The runtime reads the variable when it initialises, so it is a DEPLOYMENT setting
// (GPU_MAX_HW_QUEUES in the environment of the process); the library does not touch the environment.  What it does instead: the first batch
// that runs two sub-batch streams brackets them with events, the next call reads the overlap (bn254_groth16_stream_overlap), and a device whose sub-batch streams
// were found to run one after the other gets one sub-batch per launch from then on (same work, fewer launches) and a line in bn254_last_diagnostic().
static thread_local std::string g_diag;
void set_diag(const std::string& msg) { g_diag = msg; }
static std::atomic<int> g_profiling{0};
static std::atomic<unsigned> g_prof_mask{0xffffffffu};
static std::atomic<unsigned> g_prof_epoch{0};   // bumped by the two profiling setters: an accumulating profile (mode 2) starts over at the next batch
// Knobs of the RLC batch mode.  Initial values come from the environment (env_long); afterwards only bn254_set_rlc_params changes them.
#define RLC_MIN_BATCH 64            // below this the mode has no groups to speak of
#define RLC_PAYS_FROM 200000        // the mode is a longer pipeline (~18 ms whatever the size): measured 0.12 x at 4096, 0.45 x at 16384, 0.94 x at 2^17, 2.0 x at 2^20
static std::atomic<long> g_rlc_min_batch{[] { long v = env_long("BN254_RLC_MIN_BATCH", RLC_PAYS_FROM); return v < RLC_MIN_BATCH ? (long)RLC_MIN_BATCH : v; }()};
static std::atomic<int> g_rlc_adaptive{env_long("BN254_RLC_ADAPTIVE", 1) != 0 ? 1 : 0};
static std::atomic<long> g_rlc_share_min_lanes{env_long("BN254_RLC_SHARE_MIN_LANES", 65536)};
// Keys with more than RLC_MAX_PUBLIC inputs do their public-input MSM once per group instead of once per proof (bn254_rlc.h, group scalars), and that MSM is most
// of an exact pass at large widths: there the mode pays from far fewer proofs.  Measured crossovers, all proofs valid (profiles/r06_rlc_wide_vs_exact.txt): about
// 9 500 proofs at 1024 inputs, 15 000 at 512, 26 000 at 256, 50 000 at 128, 90 000 at 40, 140 000 at 9 and 16 -- fitted (conservatively below 128) by
// RLC_WIDE_PAYS_FIXED + RLC_WIDE_PAYS_SCALE / n_public.  BN254_RLC_WIDE_MIN_BATCH in the environment at load time replaces the fit by one value for every such key.
// A wide key honours the flag from the smaller of that and the threshold above, so bn254_set_rlc_params(64, ...) lowers both, and the default of the one above
// (RLC_PAYS_FROM) caps the fit for narrow-ish keys.
#define RLC_WIDE_PAYS_FIXED 4096
#define RLC_WIDE_PAYS_SCALE 6000000
static const long g_rlc_wide_min_batch_env = [] { long v = env_long("BN254_RLC_WIDE_MIN_BATCH", -1); return v < 0 ? -1L : (v < RLC_MIN_BATCH ? (long)RLC_MIN_BATCH : v); }();
static long rlc_wide_pays_from(size_t n_public) {
  return g_rlc_wide_min_batch_env >= 0 ? g_rlc_wide_min_batch_env : (long)(RLC_WIDE_PAYS_FIXED + RLC_WIDE_PAYS_SCALE / (n_public ? n_public : 1));
}

DevState* dev_state(const bn254_g16_pvk* pvk, int device) {
  std::lock_guard<std::mutex> lk(pvk->mu);
  return &pvk->dev[device];   // std::map nodes never move
}
// caller holds d.mu
int ensure_dev(const bn254_g16_pvk* pvk, DevState& d, int device, size_t n) {
  int rc = check_device(device);
  if (rc || (rc = selftest_gate(device))) return rc;
  if (!d.ready) {
    if ((rc = upload(d.k0, pvk->host.k0)) || (rc = upload(d.gtab, pvk->host.gtab)) || (rc = upload(d.dtab, pvk->host.dtab)) || (rc = upload(d.target, pvk->host.target)))
      return rc;
    // comb tables above 16 inputs; 13-bit windows (bn254_fw.h) up to 16; byte windows only for the diagnostic BN254_WIDE_COMB=0 (k_g16_msm_partial)
    if (!pvk->host.kpts.empty() && pvk->host.msm.empty()) { if ((rc = build_tables_on_device(g16_table_form(pvk->host), pvk->host.kpts, d.msm))) return rc; }
    else if ((rc = upload(d.msm, pvk->host.msm))) return rc;
    if ((rc = d.busy_ev.ensure())) return rc;
    d.ready = true;
  }
  // what a reservation of n proofs needs (bn254_g16_plan.h: the same function the plan probe and its property test read)
  const G16Alloc need = g16_alloc_for(n, pvk->host.key_inputs(), pvk->host.msm_comb);
  if ((rc = d.ws.ensure(need.ws_proofs * (size_t)(G16_WS_BYTES_PER_PROOF / 4)))) return rc;
  // launches that compact run on slots: slot -> proof, slot status bytes and the block counts, for as many proofs as the workspace holds
  if (need.ws_proofs > d.compact_cap) {
    const G16CompactAlloc ca = g16_compact_alloc(need.ws_proofs, pvk->host.key_inputs());
    if (g16_key_may_compact(pvk->host.key_inputs())) {
      d.compact_cap = 0;
      if ((rc = d.compact.ensure((ca.slot_proof_bytes + ca.count_bytes + ca.slot_status_bytes + 3) / 4))) return rc;
      d.compact_cap = need.ws_proofs;
    }
  }
  // keys with many public inputs: partial sums (and comb digits) of the public-input MSM, for the proofs of one launch.  Sized HERE (reserve /
  // the entry points call ensure_dev before they enqueue), so that the enqueue path itself never allocates or frees
  if (need.msm_part_proofs > d.msm_part_cap) {
    d.msm_part_cap = 0;
    if ((rc = d.msm_part.ensure((need.msm_part_bytes + need.msm_digit_bytes + 3) / 4))) return rc;
    d.msm_part_cap = need.msm_part_proofs; d.msm_chunks = need.msm_chunks;
  }
  if (g_profiling.load() && !d.ev_ready) {
    for (auto& e : d.ev) if ((rc = e.ensure_timed())) return rc;
    const int cap = 1024;  // launches per sub-batch: ~720
    for (G16ProfPool& p : d.prof) {
      p.own.resize(2 * cap); p.ev.resize(2 * cap); p.kid.resize(cap);
      for (int i = 0; i < 2 * cap; i++) { if ((rc = p.own[i].ensure_timed())) return rc; p.ev[i] = p.own[i]; }
      p.prof.ev = p.ev.data(); p.prof.kid = p.kid.data(); p.prof.cap = cap;
    }
    d.ev_ready = true;
  }
  return BN254_OK;
}
// BN254_FLAG_COMPRESSED_PROOFS / SP1 public inputs: the decompression scratch and the row scratch for a batch of n proofs (caller holds d.mu).  Grown here, by the
// entry points before they enqueue, never by the enqueue path: such a batch allocates only when it is larger than every one before it on this (key, device)
static int ensure_scratch(DevState& d, size_t n, unsigned flags, bool sp1) {
  int rc;
  if (flags & BN254_FLAG_COMPRESSED_PROOFS) { const G16CmpAlloc need = g16_cmp_alloc(n); if ((rc = d.cmp.ensure(need.raw_bytes + need.pre_bytes))) return rc; }
  if (sp1) { const G16Sp1Alloc need = g16_sp1_alloc(n); if ((rc = d.sp1.ensure(need.row_bytes + need.pre_bytes))) return rc; }
  return BN254_OK;
}
// The sub-batches of a chunk that run side by side: part pi on slot pi % 4, slot 0 = the caller's stream, slots 1..3 = the auxiliary streams (created here, when a
// batch first needs them).  parts_fork records where they start; part_begin makes an auxiliary stream wait for that point; part_join makes the caller's stream wait for
// the last part of every auxiliary stream.
static int ensure_aux(DevState& d, int count) {
  int rc;
  if ((rc = d.fork_ev.ensure())) return rc;
  for (auto& e : d.join_ev) if ((rc = e.ensure())) return rc;
  for (int i = 0; i < count && i < 3; i++) if ((rc = d.aux[i].ensure())) return rc;
  return BN254_OK;
}
static int parts_fork(DevState& d, hipStream_t user, int parts) {
  int rc = ensure_aux(d, parts - 1);
  if (rc) return rc;
  HIPCK(hipEventRecord(d.fork_ev, user));
  return BN254_OK;
}
static int part_begin(DevState& d, hipStream_t user, bool concurrent, int pi, hipStream_t* st) {
  *st = (concurrent && pi % 4) ? (hipStream_t)d.aux[pi % 4 - 1] : user;
  if (concurrent && pi < 4 && *st != user) HIPCK(hipStreamWaitEvent(*st, d.fork_ev, 0));
  return BN254_OK;
}
static int part_join(DevState& d, hipStream_t user, bool concurrent, int pi, int parts, hipStream_t st) {
  if (concurrent && (pi + 4 >= parts) && st != user) { HIPCK(hipEventRecord(d.join_ev[pi % 4], st)); HIPCK(hipStreamWaitEvent(user, d.join_ev[pi % 4], 0)); }
  return BN254_OK;
}

static KeyCache<bn254_g16_pvk, bn254_groth16_vk_free>& g16_key_cache() { static auto* c = new KeyCache<bn254_g16_pvk, bn254_groth16_vk_free>(); return *c; }

extern "C" {

void bn254_set_profiling(int enabled) { g_profiling.store(enabled); g_prof_epoch++; }
void bn254_set_profile_kernels(unsigned mask) { g_prof_mask.store(mask); g_prof_epoch++; }
int bn254_groth16_num_kernel_kinds(void) { return KID_COUNT; }
const char* bn254_groth16_kernel_kind_name(int i) {
  if (i == KID_MSM_PARTIAL) { const char* e = getenv("BN254_WIDE_COMB"); if (!(e && atoi(e) == 0)) return "k_g16_msm_partial_comb"; }   // the table form in use
  return (i >= 0 && i < KID_COUNT) ? bn254_kernel_kind_names[i] : "";
}
const char* bn254_groth16_kernel_name(int i) {
  static const char* names[BN254_G16_NUM_KERNELS] = {"phase_prepare", "phase_miller", "phase_subgroup", "phase_finalexp"};
  return (i >= 0 && i < BN254_G16_NUM_KERNELS) ? names[i] : "";
}

int bn254_groth16_vk_prepare(const uint8_t* vk, size_t vk_len, unsigned mode, bn254_g16_pvk** out) {
  if (!vk || !out || mode > 1) return set_err(BN254_E_BAD_ARG, "bad argument");
  *out = nullptr;
  G16Key key;
  if (parse_g16_vk(key, vk, vk_len, (int)mode) != DEC_OK) return set_err(BN254_E_VK, "verifying key does not parse");
  bn254_g16_pvk* p = new (std::nothrow) bn254_g16_pvk();
  if (!p) return set_err(BN254_E_NOMEM, "out of memory");
  if (!prepare_g16(p->host, key, (int)mode)) { delete p; return set_err(BN254_E_VK, "no line table for a G2 element of the key (unreachable for a point on the twist: bn254_host.hpp::prepare_g16)"); }
  *out = p;
  return BN254_OK;
}
void bn254_groth16_vk_free(bn254_g16_pvk* pvk) {
  if (!pvk) return;
  keys_sets_drop(pvk);     // cached key sets that contain the key hold copies of its tables and its handle
  for (auto it = pvk->dev.begin(); it != pvk->dev.end();) {
    if (hipSetDevice(it->first) != hipSuccess) { ++it; continue; }   // (its state goes with the key below, without the wait)
    (void)hipDeviceSynchronize();
    it = pvk->dev.erase(it);      // the state's members release what they own on the device that is now current and idle
  }
  delete pvk;
}
size_t bn254_groth16_vk_num_public(const bn254_g16_pvk* pvk) { return pvk ? (pvk->host.n_k ? pvk->host.n_k - 1 : (size_t)-1) : 0; }

int bn254_groth16_reserve(const bn254_g16_pvk* pvk, size_t n, int device) {
  if (!pvk) return set_err(BN254_E_BAD_ARG, "null key");
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  return ensure_dev(pvk, *d, device, n ? n : 1);
}

}  // extern "C"

// What both enqueue paths hand a launch part in the same way: proofs [off + lo, off + lo + count) of the batch, at `lo` in the chunk's workspace.  Each path adds what
// differs: inputs_match_key, part_of_larger, the partial-sum buffer of a wide key, the compaction slots, the split streams
static G16LaunchArgs g16_part_args(const bn254_g16_pvk* pvk, DevState* d, const void* d_proofs, size_t proof_stride, const void* d_inputs, size_t n_public, size_t off,
                                   size_t lo, size_t count, void* d_status, unsigned flags) {
  G16LaunchArgs a;
  a.proofs = (const uint8_t*)d_proofs + (off + lo) * proof_stride; a.stride = proof_stride;
  a.inputs = (const uint8_t*)d_inputs + (off + lo) * n_public * 32; a.n_public = (int)n_public; a.n = count;
  a.ws = d->ws + lo * (size_t)(G16_WS_BYTES_PER_PROOF / 4); a.status = (uint8_t*)d_status + off + lo; a.msm_tab = d->msm; a.k0 = d->k0;
  a.gtab = d->gtab; a.dtab = d->dtab; a.target = d->target;
  a.strict_scalars = (flags & BN254_FLAG_STRICT_SCALARS) ? 1 : 0;
  a.msm_comb = pvk->host.msm_comb ? 1 : 0; a.msm_part = nullptr;
  a.key_inputs = pvk->host.key_inputs(); a.rlc = (flags & BN254_FLAG_RLC) ? 1 : 0;
  return a;
}

// Enqueue the exact pipeline for n proofs on `user`.  Caller holds d->mu and has called ensure_dev.
static int g16_enqueue_exact(const bn254_g16_pvk* pvk, DevState* d, const void* d_proofs, size_t proof_stride, const void* d_inputs,
                             size_t n_public, size_t n, void* d_status, hipStream_t user, unsigned flags) {
  const int n_streams = sub_batch_streams();
  // BN254_CHUNK_LOG2 (experiment): proofs per workspace chunk, default 2^20
  static const size_t chunk = [] { const char* e = getenv("BN254_CHUNK_LOG2"); int v = e ? atoi(e) : 20; if (v < 12) v = 12; if (v > 20) v = 20; return (size_t)1 << v; }();
  const int profiling = g_profiling.load();
  // the overlap of the sub-batch streams, measured on an earlier batch: read it once it is there (no waiting)
  OvVote& ov = d->ov;
  if (ov.state == 1 && hipEventQuery(d->ov_ev[1]) == hipSuccess && hipEventQuery(d->ov_ev[3]) == hipSuccess) {
    static const bool fallback = [] { const char* e = getenv("BN254_STREAM_FALLBACK"); return !e || atoi(e) != 0; }();
    float a0 = 0, a1 = 0, s1 = 0, e1 = 0;
    const bool timed = hipEventElapsedTime(&a0, d->ov_ev[0], d->ov_ev[1]) == hipSuccess && hipEventElapsedTime(&a1, d->ov_ev[2], d->ov_ev[3]) == hipSuccess &&
                       hipEventElapsedTime(&s1, d->ov_ev[0], d->ov_ev[2]) == hipSuccess && hipEventElapsedTime(&e1, d->ov_ev[0], d->ov_ev[3]) == hipSuccess;
    const float ratio = timed ? ov_ratio(a0, a1, s1, e1) : 0.f;
    const OvChange change = ov_read(ov, timed ? &ratio : nullptr, fallback);
    if (change == OV_SERIALISED)
      ov.diag = "the two sub-batch streams of a Groth16 batch ran one after the other on this device (overlap " + std::to_string(ov.ratio) + ", " +
                std::to_string(ov.serial_votes) + " measurements in a row): the process's streams share a hardware queue -- give it more queues (GPU_MAX_HW_QUEUES, read when the HIP runtime "
                "initialises; INTEGRATION.md)" + (fallback ? "; using one sub-batch per launch, re-measured every " + std::to_string(OV_REPROBE) + " batches" : "");
    else if (change == OV_RESTORED) ov.diag = "the sub-batch streams overlap again (" + std::to_string(ov.ratio) + "): back to two sub-batches side by side";
  }
  const bool probe_now = ov_begin_batch(ov);                            // a re-probe runs two streams again and is measured
  const bool single_stream = ov.single_stream && !probe_now;
  for (size_t off = 0; off < n; off += chunk) {
    size_t m = n - off < chunk ? n - off : chunk;
    G16ChunkPlan plan;
    if (!g16_plan_chunk(plan, m, pvk->host.key_inputs(), n_public, n_streams, single_stream)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
    const bool wide = plan.wide, concurrent = plan.concurrent, split_small = plan.split_small;
    const int parts = plan.parts;
    // the buffers were sized by ensure_dev (bn254_groth16_reserve or the entry point itself): this path only enqueues, after checking the plan against them
    if (m > d->ws_proofs()) return set_err(BN254_E_BAD_ARG, "workspace smaller than the batch: bn254_groth16_reserve first");
    if (wide) for (int pi = 0; pi < parts; pi++)
      if (plan.part[pi].count > d->msm_part_cap) return set_err(BN254_E_BAD_ARG, "workspace of a key with many public inputs is smaller than the batch: bn254_groth16_reserve first");
    int rc;
    if ((rc = concurrent ? parts_fork(*d, user, parts) : split_small ? ensure_aux(*d, 2) : BN254_OK)) return rc;
    const bool measure_overlap = ov_measures(ov, concurrent, parts, plan.part[0].count, parts >= 2 ? plan.part[1].count : 0);
    if (measure_overlap) for (auto& e : d->ov_ev) if ((rc = e.ensure_timed())) return rc;
    for (int pi = 0; pi < parts; pi++) {
      const size_t lo = plan.part[pi].first;
      hipStream_t st;
      if ((rc = part_begin(*d, user, concurrent, pi, &st))) return rc;
      if (measure_overlap && pi < 2) HIPCK(hipEventRecord(d->ov_ev[2 * pi], st));
      G16LaunchArgs a = g16_part_args(pvk, d, d_proofs, proof_stride, d_inputs, n_public, off, lo, plan.part[pi].count, d_status, flags);
      a.inputs_match_key = pvk->host.inputs_match(n_public) ? 1 : 0;
      a.part_of_larger = parts > 1 ? 1 : 0;
      if (wide) a.msm_part = (int32_t*)d->msm_part;
      if (wide && pvk->host.msm_comb) a.msm_digits = (uint16_t*)(d->msm_part + d->msm_chunks * 27 * d->msm_part_cap);
      // the slots of a launch that compacts (bn254_launch_g16 decides with g16_compacts, from the form it takes): the part's share of the three arrays, at its first
      // proof like its share of the workspace.  The context of a key that may compact holds them for as many proofs as its workspace (ensure_dev): a smaller one is a
      // sizing error, not a reason to run without compaction
      if (g16_key_may_compact(a.key_inputs)) {
        if (m > d->compact_cap) return set_err(BN254_E_BAD_ARG, "slot arrays smaller than the batch: bn254_groth16_reserve first");
        const G16CompactAlloc ca = g16_compact_alloc(d->compact_cap, a.key_inputs);
        a.slot_proof = (uint32_t*)d->compact + lo;
        a.block_count = (uint32_t*)d->compact + ca.slot_proof_bytes / 4 + lo / G16_COMPACT_BLOCK;
        a.slot_status = (uint8_t*)((uint32_t*)d->compact + (ca.slot_proof_bytes + ca.count_bytes) / 4) + lo;
      }
      if (split_small && parts == 1) {
        a.split_streams[0] = d->aux[0]; a.split_streams[1] = d->aux[1];
        a.split_ev[0] = d->fork_ev; a.split_ev[1] = d->join_ev[1]; a.split_ev[2] = d->join_ev[2];
      }
      // the first two parts record per-launch event pairs, each into its pool; the phase events bracket the kernels of part 0 of the LAST chunk only (one chunk
      // for n <= 2^20).  Mode 1: the event pairs of THIS batch; mode 2: the pairs accumulate over the batches enqueued since the last call of a profiling setter (a
      // caller that times many back-to-back batches reads them once at the end instead of synchronising with every batch; a full pool simply stops recording)
      G16Prof* prof = profiling && d->ev_ready && pi < 2 ? &d->prof[pi].prof : nullptr;
      if (prof) {
        const unsigned epoch = g_prof_epoch.load();
        const bool keep = profiling == 2 && d->prof_epoch == epoch && d->prof[0].prof.used > 0;
        prof->mask = g_prof_mask.load();
        if (!keep) prof->used = 0;
        if (pi == 0) { d->prof_n = a.n; d->prof_epoch = epoch; if (!keep) d->prof[1].prof.used = 0; }
        d->prof2_used = pi == 1 || (keep && d->prof2_used);
      }
      hipEvent_t phase_ev[5];
      for (int k = 0; k < 5; k++) phase_ev[k] = d->ev[k];
      hipError_t e = bn254_launch_g16(a, st, prof && pi == 0 ? phase_ev : nullptr, prof);
      if (e != hipSuccess) return launch_err(e, nullptr);
      if (measure_overlap && pi < 2) HIPCK(hipEventRecord(d->ov_ev[2 * pi + 1], st));
      if ((rc = part_join(*d, user, concurrent, pi, parts, st))) return rc;
    }
    if (measure_overlap) ov.state = 1;
  }
  d->ev_recorded = profiling && d->ev_ready;
  return BN254_OK;
}

// ---- BN254_FLAG_RLC (bn254_rlc.h): first pass in groups, exact second pass over the proofs of groups that failed -----------------------------
// n: proofs of the chunk; plan: its launch parts (the wide buffers hold plan.wide_groups groups)
static int rlc_ensure(const bn254_g16_pvk* pvk, DevState* d, size_t n, size_t n_public, const G16RlcChunkPlan& plan) {
  RlcDev& r = d->rlc;
  int rc;
  if (!r.ready) {
    {
      std::lock_guard<std::mutex> lk(pvk->mu);
      if (!pvk->rlc_host.ready && !prepare_g16_rlc(pvk->rlc_host, pvk->host)) return set_err(BN254_E_VK, "degenerate key element (RLC tables)");
    }
    if ((rc = upload(r.btab, pvk->rlc_host.btab)) || (rc = upload(r.one, pvk->rlc_host.one))) return rc;
    if ((rc = build_tables_on_device(2, pvk->rlc_host.pts, r.tab))) return rc;      // -alpha and K[0]: 13-bit windows like the key's own (vm_rlc_group_points reads both)
    r.ready = true;
  }
  if (n > r.grp_cap) {   // the four are sized together: grp_cap is what ALL of them hold, 0 while any of them is being replaced
    r.grp_cap = 0;
    const size_t cap = g16_rlc_alloc(n);               // group status regions of the launch parts are rounded up to 256 each (bn254_g16_plan.h)
    if ((rc = r.grp_status.ensure(cap)) || (rc = r.idx.ensure(cap)) || (rc = r.h_status.ensure(cap)) || (rc = r.h_idx.ensure(cap))) return rc;
    r.grp_cap = n;
  }
  if (n_public > (size_t)RLC_MAX_PUBLIC && plan.wide_groups > r.wide_cap) {   // likewise, for wide_cap groups
    r.wide_cap = 0;
    const size_t cap = g16_round256(plan.wide_groups);
    const G16RlcWide a = g16_rlc_wide_alloc(cap, n_public, g16_table_form(pvk->host));
    if ((rc = r.grp_rows.ensure(a.rows_bytes)) || (a.digit_bytes && (rc = r.grp_digits.ensure((a.digit_bytes + 1) / 2))) || (a.part_bytes && (rc = r.grp_part.ensure((a.part_bytes + 3) / 4))))
      return rc;
    r.wide_cap = cap;
  }
  return BN254_OK;
}
// The RLC plan of a chunk of m proofs under the knobs as they stand: the ONE reading of BN254_RLC_GROUP_LOG2, BN254_RLC_SHARE_LOG2 (once per process), BN254_STREAMS
// and share_min_lanes (bn254_set_rlc_params may run beside a batch: one load per chunk).  g16_enqueue_rlc launches by it; bn254_dbg_g16_rlc_groups shows it.
static bool g16_rlc_chunk_plan_now(G16RlcChunkPlan& plan, size_t m) {
  static const int log2_group = [] { const char* e = getenv("BN254_RLC_GROUP_LOG2"); int v = e ? atoi(e) : 5; return v < 1 ? 1 : (v > 16 ? 16 : v); }();
  // proofs per lane in the Miller loop (shared accumulator, one squaring of f per lane and step): 2^BN254_RLC_SHARE_LOG2, at most the group
  static const int log2_share_env = [] { const char* e = getenv("BN254_RLC_SHARE_LOG2"); int v = e ? atoi(e) : 3; return v < 0 ? 0 : (v > 3 ? 3 : v); }();
  const long ml = g_rlc_share_min_lanes.load();
  return g16_plan_rlc_chunk(plan, m, sub_batch_streams(), log2_group, log2_share_env, ml < 1 ? 1 : (size_t)ml);
}
static int g16_enqueue_rlc(const bn254_g16_pvk* pvk, DevState* d, int device, const void* d_proofs, size_t proof_stride, const void* d_inputs,
                           size_t n_public, size_t n, void* d_status, hipStream_t user, unsigned flags) {
  (void)device;
  uint32_t key[11];
  if (getrandom(key, sizeof key, 0) != (ssize_t)sizeof key) return set_err(BN254_E_HIP, "getrandom failed: no weights for the RLC mode");
  size_t seen_checked = 0, seen_fallback = 0;
  const size_t chunk = G16_MAX_BATCH;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = n - off < chunk ? n - off : chunk;
    // ONE plan per chunk (and one reading of the knob: bn254_set_rlc_params may run beside this call): what rlc_ensure sizes for is what the parts address
    G16RlcChunkPlan plan;
    if (!g16_rlc_chunk_plan_now(plan, m)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
    const bool wide = n_public > (size_t)RLC_MAX_PUBLIC;
    int rc = rlc_ensure(pvk, d, m, n_public, plan);
    if (rc) return rc;
    RlcDev& r = d->rlc;
    if (plan.need > g16_rlc_alloc(r.grp_cap)) return set_err(BN254_E_HIP, "RLC group buffer smaller than the batch (internal sizing error)");
    if (wide && plan.wide_groups > r.wide_cap) return set_err(BN254_E_HIP, "RLC group scalar buffer smaller than the batch (internal sizing error)");
    const int msm_form = g16_table_form(pvk->host), parts = plan.parts;
    const size_t chunks_w = (n_public + G16_WIDE_MSM_INPUTS_PER_LANE - 1) / G16_WIDE_MSM_INPUTS_PER_LANE;
    const bool concurrent = parts > 1;
    if (concurrent && (rc = parts_fork(*d, user, parts))) return rc;
    for (int pi = 0; pi < parts; pi++) {
      const G16RlcPart& q = plan.part[pi];
      hipStream_t st;
      if ((rc = part_begin(*d, user, concurrent, pi, &st))) return rc;
      G16LaunchArgs a = g16_part_args(pvk, d, d_proofs, proof_stride, d_inputs, n_public, off, q.first, q.count, d_status, flags);
      a.inputs_match_key = 1;
      RlcLaunchArgs ra;
      memcpy(ra.key, key, sizeof key);
      ra.counter_base = (uint32_t)(off + q.first);
      ra.plan = q.plan;
      ra.grp_status = r.grp_status + q.grp_off;
      ra.btab = r.btab; ra.rlc_tab = r.tab; ra.one = r.one;
      if (wide) {
        ra.grp_rows = r.grp_rows + q.wide_off * n_public * 32;
        ra.grp_digits = r.grp_digits ? r.grp_digits + q.wide_off * (size_t)G16_COMB_COLS * n_public : nullptr;
        ra.grp_part = r.grp_part ? r.grp_part + q.wide_off * chunks_w * 27 : nullptr;
        ra.msm_form = msm_form;
      }
      hipError_t e = bn254_launch_g16_rlc(a, ra, st);
      if (e != hipSuccess) return launch_err(e, "rlc");
      if ((rc = part_join(*d, user, concurrent, pi, parts, st))) return rc;
    }
    // which proofs are still pending (their group's product was not one)?  One stream synchronisation per chunk.
    HIPCK(hipMemcpyAsync(r.h_status, (const uint8_t*)d_status + off, m, hipMemcpyDeviceToHost, user));
    HIPCK(hipStreamSynchronize(user));
    uint32_t cnt = 0;
    for (size_t i = 0; i < m; i++) {
      if (r.h_status[i] == BN254_ST_PENDING) r.h_idx[cnt++] = (uint32_t)i;
      else if (r.h_status[i] == BN254_ST_ACCEPT) seen_checked++;
    }
    seen_checked += cnt; seen_fallback += cnt;
    if (cnt == 0) continue;
    if (cnt > r.fb_cap || (size_t)cnt * n_public * 32 > r.fb_in_cap) {   // the three together, released first (this key may meet other input counts)
      r.fb_cap = r.fb_in_cap = 0;
      r.fb_proofs.release(); r.fb_inputs.release(); r.fb_status.release();
      const size_t cap = ((size_t)cnt + 4095) / 4096 * 4096;
      if ((rc = r.fb_proofs.ensure(cap * 256)) || (rc = r.fb_inputs.ensure(cap * (n_public ? n_public : 1) * 32)) || (rc = r.fb_status.ensure(cap))) return rc;
      r.fb_cap = cap; r.fb_in_cap = cap * n_public * 32;
    }
    HIPCK(hipMemcpyAsync(r.idx, r.h_idx, (size_t)cnt * sizeof(uint32_t), hipMemcpyHostToDevice, user));
    hipError_t e = bn254_launch_gather_rows(r.fb_proofs, (const uint8_t*)d_proofs + off * proof_stride, proof_stride, 256, r.idx, cnt, user);
    if (e == hipSuccess && n_public) e = bn254_launch_gather_rows(r.fb_inputs, (const uint8_t*)d_inputs + off * n_public * 32, n_public * 32, (uint32_t)(n_public * 32), r.idx, cnt, user);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("gather launch: ") + hipGetErrorString(e));
    rc = g16_enqueue_exact(pvk, d, r.fb_proofs, 256, r.fb_inputs, n_public, cnt, r.fb_status, user, flags);
    if (rc) return rc;
    e = bn254_launch_scatter_status((uint8_t*)d_status + off, r.fb_status, r.idx, cnt, user);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("scatter launch: ") + hipGetErrorString(e));
  }
  if (seen_checked) {
    RlcDev& r = d->rlc;
    const float share = (float)seen_fallback / (float)seen_checked;
    r.fb_share = r.have_obs ? 0.5f * r.fb_share + 0.5f * share : share;
    r.have_obs = true;
  }
  return BN254_OK;
}
// The RLC pass costs about half an exact pass and every proof of a failed group pays the exact pass on top, so the mode loses once about half
// of the proofs fall back (measured: 0.84 x at 1/16 invalid proofs and groups of 32).  While the recent share is above RLC_BYPASS_SHARE the
// batch entry points run the exact path directly (same status bytes by construction) and re-measure with an RLC pass every RLC_PROBE_EVERY calls.
// BN254_RLC_ADAPTIVE=0 switches this off.
#define RLC_BYPASS_SHARE 0.45f
#define RLC_PROBE_EVERY 8
static bool rlc_bypass(RlcDev& r) {
  const bool adaptive = g_rlc_adaptive.load() != 0;   // bn254_set_rlc_params
  if (!adaptive || !r.have_obs || r.fb_share <= RLC_BYPASS_SHARE) { r.bypassed = 0; return false; }
  if (r.bypassed + 1 >= RLC_PROBE_EVERY) { r.bypassed = 0; return false; }
  r.bypassed++; r.bypassed_total++;
  return true;
}
// does a batch of this shape qualify for the RLC mode at all (the adaptive bypass, rlc_bypass, is decided separately, once per call)
static bool rlc_eligible(const bn254_g16_pvk* pvk, size_t n_public, size_t n, unsigned flags) {
  long from = g_rlc_min_batch.load();
  if (n_public > (size_t)RLC_MAX_PUBLIC) { const long wide_from = rlc_wide_pays_from(n_public); if (wide_from < from) from = wide_from; }
  return (flags & BN254_FLAG_RLC) && pvk->host.inputs_match(n_public) && n >= (size_t)from;
}
// BN254_FLAG_COMPRESSED_PROOFS, chunk by chunk (at most G16_MAX_BATCH proofs, the chunk of both pipelines): k_g16_decompress writes the raw records and the
// pre-status bytes into the scratch, the raw pipeline chosen for the whole batch runs on the scratch at stride 256 with the flag cleared, and k_g16_status_merge
// makes MALFORMED override.  A record that does not decompress becomes all ones, which the loader refuses with NOT_MEMBER at its first test: the proof is then
// no longer pending, so it contributes the neutral element to its RLC group and never sends the group to the exact fallback.  Everything is enqueued on `user`
// (the sub-batch streams of the exact path join it), so the next chunk's decompression overwrites the scratch only after this chunk is done with it.
static int g16_enqueue_compressed(const bn254_g16_pvk* pvk, DevState* d, int device, const void* d_proofs, size_t proof_stride, const void* d_inputs,
                                  size_t n_public, size_t n, void* d_status, hipStream_t user, unsigned flags, bool rlc) {
  const unsigned raw_flags = flags & ~(unsigned)BN254_FLAG_COMPRESSED_PROOFS;
  for (size_t off = 0; off < n; off += G16_MAX_BATCH) {
    const size_t m = n - off < (size_t)G16_MAX_BATCH ? n - off : (size_t)G16_MAX_BATCH;
    if (g16_cmp_alloc(m).proofs > d->cmp_proofs()) return set_err(BN254_E_BAD_ARG, "decompression scratch smaller than the batch (internal sizing error)");
    uint8_t* raw = d->cmp;
    uint8_t* pre = d->cmp + d->cmp_proofs() * 256;
    uint8_t* st = (uint8_t*)d_status + off;
    const uint8_t* in = (const uint8_t*)d_inputs + off * n_public * 32;
    hipError_t e = bn254_launch_g16_decompress((const uint8_t*)d_proofs + off * proof_stride, proof_stride, (uint32_t)m, raw, pre, user);
    if (e != hipSuccess) return launch_err(e, "decompress");
    int rc = rlc ? g16_enqueue_rlc(pvk, d, device, raw, 256, in, n_public, m, st, user, raw_flags)
                 : g16_enqueue_exact(pvk, d, raw, 256, in, n_public, m, st, user, raw_flags);
    if (rc) return rc;
    e = bn254_launch_g16_status_merge(st, pre, (uint32_t)m, user);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("kernel launch (status merge): ") + hipGetErrorString(e));
  }
  return BN254_OK;
}
// the pipeline of one batch (or of one chunk of SP1 rows) on `user`
static int g16_dispatch(const bn254_g16_pvk* pvk, DevState* d, int device, const void* d_proofs, size_t proof_stride, const void* d_inputs, size_t n_public, size_t n,
                        void* d_status, hipStream_t user, unsigned flags, bool rlc) {
  if (flags & BN254_FLAG_COMPRESSED_PROOFS) return g16_enqueue_compressed(pvk, d, device, d_proofs, proof_stride, d_inputs, n_public, n, d_status, user, flags, rlc);
  return rlc ? g16_enqueue_rlc(pvk, d, device, d_proofs, proof_stride, d_inputs, n_public, n, d_status, user, flags)
             : g16_enqueue_exact(pvk, d, d_proofs, proof_stride, d_inputs, n_public, n, d_status, user, flags);
}
// one batch on `user`: waits for the previous batch of this (key, device), runs the exact or the RLC pipeline, records busy_ev.
// use_rlc: -1 = decide here; 0 / 1 = the caller (the host-buffer entry, which must know before it cuts the batch into chunks) has decided.
// sp1 != nullptr, SP1 public inputs (d_inputs is not read, n_public is 2), chunk by chunk (at most G16_MAX_BATCH proofs, as g16_enqueue_compressed):
// k_sp1_public_inputs writes the rows vkey_hash | digest and the pre-status bytes into the row scratch, the pipeline chosen for the whole batch (with
// BN254_FLAG_COMPRESSED_PROOFS: decompression first) runs on the rows, and k_g16_status_merge makes MALFORMED override for a range outside the values buffer.
// Everything is on `user`, so the next chunk's hashing overwrites the rows only after this chunk is done with them.
static int g16_enqueue(const bn254_g16_pvk* pvk, DevState* d, int device, const void* d_proofs, size_t proof_stride, const void* d_inputs,
                       size_t n_public, size_t n, void* d_status, hipStream_t user, unsigned flags, int use_rlc = -1, const Sp1Src* sp1 = nullptr) {
  if (sp1) n_public = 2;
  if (d->busy_valid) HIPCK(hipStreamWaitEvent(user, d->busy_ev, 0));
  int rc = BN254_OK;
  // BN254_FLAG_RLC is honoured where it pays: from RLC_PAYS_FROM proofs (bn254_set_rlc_params / BN254_RLC_MIN_BATCH at load time move the
  // threshold: the tests run the mode on small batches); smaller batches take the exact path -- same status bytes
  const bool rlc = use_rlc >= 0 ? use_rlc != 0 : (rlc_eligible(pvk, n_public, n, flags) && !rlc_bypass(d->rlc));
  if (!sp1) rc = g16_dispatch(pvk, d, device, d_proofs, proof_stride, d_inputs, n_public, n, d_status, user, flags, rlc);
  else for (size_t off = 0; off < n; off += G16_MAX_BATCH) {
    const size_t m = n - off < (size_t)G16_MAX_BATCH ? n - off : (size_t)G16_MAX_BATCH;
    if (g16_sp1_alloc(m).proofs > d->sp1_proofs()) return set_err(BN254_E_BAD_ARG, "SP1 row scratch smaller than the batch (internal sizing error)");
    uint8_t* rows = d->sp1;
    uint8_t* pre = d->sp1 + d->sp1_proofs() * 64;
    uint8_t* st = (uint8_t*)d_status + off;
    hipError_t e = bn254_launch_sp1_public_inputs(sp1->vkh + off * sp1->vkh_stride, sp1->vkh_stride, sp1->pv, sp1->pv_bytes, sp1->pv_base, sp1->off + off, (uint32_t)m, rows, pre, user);
    if (e != hipSuccess) return launch_err(e, "SP1 public inputs");
    if ((rc = g16_dispatch(pvk, d, device, (const uint8_t*)d_proofs + off * proof_stride, proof_stride, rows, 2, m, st, user, flags, rlc))) return rc;
    if ((e = bn254_launch_g16_status_merge(st, pre, (uint32_t)m, user)) != hipSuccess) return set_err(BN254_E_HIP, std::string("kernel launch (status merge): ") + hipGetErrorString(e));
  }
  if (rc) return rc;
  HIPCK(hipEventRecord(d->busy_ev, user));
  d->busy_valid = true;
  return BN254_OK;
}
int g16_sp1_device(const bn254_g16_pvk* pvk, const void* d_proofs, size_t proof_stride, const Sp1Src& s, size_t n, void* d_status, int device, hipStream_t user, unsigned flags) {
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  int rc;
  if ((rc = ensure_dev(pvk, *d, device, n)) || (rc = ensure_scratch(*d, n, flags, true))) return rc;
  return g16_enqueue(pvk, d, device, d_proofs, proof_stride, nullptr, 2, n, d_status, user, flags, -1, &s);
}

extern "C" {

int bn254_groth16_verify_batch_device(const bn254_g16_pvk* pvk, const void* d_proofs, size_t proof_stride, const void* d_inputs,
                                      size_t n_public, size_t n, void* d_status, int device, void* hip_stream, unsigned flags) {
  int rc = check_batch_args(false, pvk, d_proofs, proof_stride, d_inputs, n_public, n, d_status, flags);
  if (rc || n == 0) return rc;
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  if ((rc = ensure_dev(pvk, *d, device, n)) || (rc = ensure_scratch(*d, n, flags, false))) return rc;
  return g16_enqueue(pvk, d, device, d_proofs, proof_stride, d_inputs, n_public, n, d_status, (hipStream_t)hip_stream, flags);
}

void bn254_set_rlc_params(long min_batch, int adaptive, long share_min_lanes) {
  if (min_batch >= 0) g_rlc_min_batch.store(min_batch < RLC_MIN_BATCH ? (long)RLC_MIN_BATCH : min_batch);
  if (adaptive >= 0) g_rlc_adaptive.store(adaptive ? 1 : 0);
  if (share_min_lanes >= 0) g_rlc_share_min_lanes.store(share_min_lanes < 1 ? 1 : share_min_lanes);
}

// Host-only probe: the groups a chunk of m proofs forms under BN254_FLAG_RLC with the knobs as they stand -- the plan g16_enqueue_rlc makes for that chunk.
// out_group[i]: proof i's group, numbered through the chunk (the groups of the launch parts before its own come first); out_log2_share[i]: its part's log2_share
int bn254_dbg_g16_rlc_groups(size_t m, unsigned* out_group, uint8_t* out_log2_share) {
  if (!out_group || !out_log2_share || m == 0 || m > (size_t)G16_MAX_BATCH) return set_err(BN254_E_BAD_ARG, "bad argument");
  G16RlcChunkPlan plan;
  if (!g16_rlc_chunk_plan_now(plan, m)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
  for (int pi = 0; pi < plan.parts; pi++) {
    const G16RlcPart& q = plan.part[pi];
    for (size_t i = 0; i < q.count; i++) {
      out_group[q.first + i] = (unsigned)q.wide_off + rlc_group_of((uint32_t)i, q.plan);
      out_log2_share[q.first + i] = (uint8_t)q.log2_share;
    }
  }
  return BN254_OK;
}

int bn254_groth16_rlc_state(const bn254_g16_pvk* pvk, int device, float* fallback_share, unsigned* bypassed_calls) {
  if (!pvk) return set_err(BN254_E_BAD_ARG, "bad argument");
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  if (fallback_share) *fallback_share = d->rlc.have_obs ? d->rlc.fb_share : -1.f;
  if (bypassed_calls) *bypassed_calls = d->rlc.bypassed_total;
  return BN254_OK;
}

const char* bn254_last_diagnostic(void) { return g_diag.c_str(); }

// How the two sub-batch streams of this (key, device) ran on the first batch that used two: sum of their durations / their union (about 2: side by side; about
// 1: one after the other, i.e. they share a hardware queue -- see GPU_MAX_HW_QUEUES in INTEGRATION.md); -1 while no such batch has been measured.
int bn254_groth16_stream_overlap(const bn254_g16_pvk* pvk, int device, float* overlap, int* single_stream) {
  if (!pvk || !overlap) return set_err(BN254_E_BAD_ARG, "bad argument");
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  *overlap = d->ov.ratio;            // -1 until the first measurement has been read
  if (single_stream) *single_stream = d->ov.single_stream ? 1 : 0;
  g_diag = d->ov.diag;               // the explanation belongs to the (key, device); the caller's thread receives it here
  return BN254_OK;
}

int bn254_groth16_last_kernel_ms(const bn254_g16_pvk* pvk, int device, float ms[BN254_G16_NUM_KERNELS]) {
  if (!pvk || !ms) return set_err(BN254_E_BAD_ARG, "bad argument");
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  if (!d->ev_recorded) return set_err(BN254_E_BAD_ARG, "no profiled batch on this device");
  HIPCK(hipSetDevice(device));
  HIPCK(hipEventSynchronize(d->ev[4]));
  for (int i = 0; i < BN254_G16_NUM_KERNELS; i++) HIPCK(hipEventElapsedTime(&ms[i], d->ev[i], d->ev[i + 1]));
  return BN254_OK;
}

}  // extern "C"

// The per-launch event pairs of the last profiled batch: launches and summed durations per kernel kind.  union_ms == nullptr: the first sub-batch alone, each launch
// from its own pair of events.  Otherwise the first TWO sub-batches (they run on two streams side by side), every launch as an interval [start, end] on a common
// time base (the first sub-batch's first event), and union_ms[k] = the length of the union of the intervals of kind k: for two streams that run the same kernel at
// the same time about one launch's duration, for launches that happen to run one after the other the sum -- either way "work of all those launches / union" is the
// rate the GPU delivered while that kernel kind was running.
static int g16_read_profile(const bn254_g16_pvk* pvk, int device, unsigned launches[], float total_ms[], float union_ms[], size_t* proofs_per_launch) {
  DevState* dp = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(dp->mu);
  DevState& d = *dp;
  if (!d.ev_recorded || (union_ms && d.prof[0].prof.used == 0)) return set_err(BN254_E_BAD_ARG, "no profiled batch on this device");
  HIPCK(hipSetDevice(device));
  std::vector<std::vector<std::pair<float, float>>> iv(KID_COUNT);
  for (int k = 0; k < KID_COUNT; k++) { launches[k] = 0; total_ms[k] = 0.f; if (union_ms) union_ms[k] = 0.f; }
  const int pools = union_ms && d.prof2_used ? 2 : 1;
  for (int pi = 0; pi < pools; pi++) {
    const G16Prof& p = d.prof[pi].prof;
    for (int i = 0; i < p.used; i++) {
      HIPCK(hipEventSynchronize(p.ev[2 * i + 1]));
      float a = 0.f, b = 0.f;
      if (union_ms) HIPCK(hipEventElapsedTime(&a, d.prof[0].prof.ev[0], p.ev[2 * i]));
      HIPCK(hipEventElapsedTime(&b, union_ms ? d.prof[0].prof.ev[0] : p.ev[2 * i], p.ev[2 * i + 1]));
      launches[p.kid[i]]++; total_ms[p.kid[i]] += b - a;
      if (union_ms) iv[p.kid[i]].push_back({a, b});
    }
  }
  for (int k = 0; union_ms && k < KID_COUNT; k++) {
    auto& v = iv[k];
    std::sort(v.begin(), v.end());
    float cur_lo = 0.f, cur_hi = 0.f; bool open = false;
    for (auto& x : v) {
      if (!open) { cur_lo = x.first; cur_hi = x.second; open = true; }
      else if (x.first <= cur_hi) { if (x.second > cur_hi) cur_hi = x.second; }
      else { union_ms[k] += cur_hi - cur_lo; cur_lo = x.first; cur_hi = x.second; }
    }
    if (open) union_ms[k] += cur_hi - cur_lo;
  }
  if (proofs_per_launch) *proofs_per_launch = d.prof_n;
  return BN254_OK;
}

extern "C" {

int bn254_groth16_kernel_profile(const bn254_g16_pvk* pvk, int device, unsigned launches[], float total_ms[], size_t* proofs_per_launch) {
  if (!pvk || !launches || !total_ms) return set_err(BN254_E_BAD_ARG, "bad argument");
  return g16_read_profile(pvk, device, launches, total_ms, nullptr, proofs_per_launch);
}
int bn254_groth16_kernel_profile_all(const bn254_g16_pvk* pvk, int device, unsigned launches[], float total_ms[], float union_ms[], size_t* proofs_per_launch) {
  if (!pvk || !launches || !total_ms || !union_ms) return set_err(BN254_E_BAD_ARG, "bad argument");
  return g16_read_profile(pvk, device, launches, total_ms, union_ms, proofs_per_launch);
}

}  // extern "C"

// Host buffers go through the key's ring of pinned pieces (PinRing, bn254_capi_owners.h): a compute chunk (2^17 proofs first, so that the exposed copy is short, then
// 2^18) waits on the GPU for the event of its last piece; one status copy at the end.  The device lock is held for the whole call: the staging buffers belong to
// this batch until its statuses are back.
// The host-buffer batch.  sp1 = nullptr: the raw entry.  sp1 != nullptr (host buffers, offsets already checked to be non-decreasing): the public inputs are the
// SP1 rows -- nothing is read from public_inputs; at the start of every compute chunk its offsets, values and vkey hashes go through the same pinned ring
// ahead of its proofs (each byte once: the values are staged as bytes [off[0], off[n]) of the caller's buffer), the chunk is hashed on the device and the
// rows never leave it.
static int g16_host_batch(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                          size_t n_public, size_t n, uint8_t* status, int device, unsigned flags, const Sp1Src* sp1) {
  int rc;
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  if ((rc = ensure_dev(pvk, *d, device, n)) || (rc = ensure_scratch(*d, n, flags, sp1 != nullptr))) return rc;
  if (sp1) n_public = 0;   // staged per proof: the proof only (the rows are made on the device)
  const size_t in_row = n_public * 32, row = proof_stride + in_row;
  size_t pb = n * proof_stride, ib = n * in_row;
  if ((rc = d->st_proofs.ensure(pb)) || (rc = d->st_inputs.ensure(ib ? ib : 32)) || (rc = d->st_status.ensure(n))) return rc;
  const uint64_t pv_total = sp1 ? sp1->off[n] - sp1->off[0] : 0;
  if (sp1 && ((rc = d->st_pv.ensure(pv_total ? pv_total : 4)) || (rc = d->st_off.ensure((n + 1) * 8)) || (rc = d->st_vkh.ensure(sp1->vkh_stride ? n * 32 : 32)))) return rc;
  // compute chunks: a short first one (its copy is the only exposed one: 2^17 proofs = 42 MB, under a millisecond of DMA), then the rest in chunks
  // as large as the workspace allows -- every chunk boundary drains both sub-batch streams, so fewer chunks is faster
  static const size_t first_chunk = [] { const char* e = getenv("BN254_HOST_FIRST_CHUNK_LOG2"); int v = e ? atoi(e) : 17; if (v < 12) v = 12; if (v > 20) v = 20; return (size_t)1 << v; }();
  const size_t hchunk = (size_t)G16_MAX_BATCH - first_chunk;
  // copy pieces: about 20 MB of the caller's bytes each (65536 proofs at 2 public inputs), a multiple of 256 proofs
  static const size_t piece_bytes_target = [] { const char* e = getenv("BN254_HOST_PIECE_MB"); long v = e ? atol(e) : 20; return (size_t)(v < 1 ? 1 : v) << 20; }();
  size_t piece = piece_bytes_target / row / 256 * 256;
  if (piece < 256) piece = 256;
  if (piece > n) piece = (n + 255) / 256 * 256;
  PinRing& ring = d->ring;
  if ((rc = ring.ensure(piece * row))) return rc;
  ring.begin();
  // the RLC mode forms its groups over the whole batch it is handed: keep it in one piece -- but only when this call really runs the mode
  // (same predicate as g16_enqueue, the adaptive bypass included, decided ONCE here); a flag that will be ignored keeps the chunked
  // copy / compute overlap
  const int use_rlc = (rlc_eligible(pvk, sp1 ? 2 : n_public, n, flags) && !rlc_bypass(d->rlc)) ? 1 : 0;
  static const bool timing = getenv("BN254_HOST_TIMING") != nullptr;   // diagnostics on stderr: where the host thread spends the call
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  double t_copy = 0, t_wait = 0, t_enq = 0;
  const auto t_begin = now();
  size_t copied = 0, computed = 0;
  // the first chunk is short (its copy is the only exposed one) unless the batch is small anyway
  size_t c_end = (use_rlc || n < 2 * first_chunk) ? n : first_chunk;
  while (computed < n) {
    if (sp1) {   // this chunk's offsets (the first chunk: off[0 .. c_end], later ones off[computed + 1 .. c_end]), values and vkey hashes
      const size_t o_lo = computed ? computed + 1 : 0;
      const uint8_t* osrc = (const uint8_t*)(sp1->off + o_lo);
      const uint64_t v_lo = sp1->off[computed] - sp1->off[0], v_hi = sp1->off[c_end] - sp1->off[0];
      const uint8_t* vsrc = sp1->pv + sp1->off[computed];
      const size_t vk_stride = sp1->vkh_stride; const uint8_t* vk = sp1->vkh; const size_t first = computed;
      if ((rc = ring.push(d->st_off + o_lo * 8, (c_end + 1 - o_lo) * 8, [&](uint8_t* q, size_t f, size_t k) { parallel_copy(q, osrc + f, k); })) ||
          (rc = ring.push(d->st_pv + v_lo, v_hi - v_lo, [&](uint8_t* q, size_t f, size_t k) { parallel_copy(q, vsrc + f, k); })))
        return rc;
      if (vk_stride == 0 && computed == 0) rc = ring.push(d->st_vkh, 32, [&](uint8_t* q, size_t, size_t) { memcpy(q, vk, 32); });
      else if (vk_stride == 32) rc = ring.push(d->st_vkh + first * 32, (c_end - first) * 32, [&](uint8_t* q, size_t f, size_t k) { parallel_copy(q, vk + first * 32 + f, k); });
      else if (vk_stride) rc = ring.push(d->st_vkh + first * 32, (c_end - first) * 32, [&](uint8_t* q, size_t f, size_t k) {
        for (size_t b = f; b < f + k;) {   // compacted to 32 bytes per proof
          const size_t r = b / 32, o = b % 32, t = 32 - o < f + k - b ? 32 - o : f + k - b;
          memcpy(q + (b - f), vk + (first + r) * vk_stride + o, t);
          b += t;
        }
      });
      if (rc) return rc;
    }
    while (copied < c_end) {   // a piece of `m` records: the proofs, then their input rows
      const size_t m = c_end - copied < piece ? c_end - copied : piece;
      uint8_t* pin;
      auto ta = now();
      if ((rc = ring.acquire(&pin))) return rc;
      auto tb = now();
      parallel_copy(pin, proofs + copied * proof_stride, m * proof_stride);
      if (in_row) parallel_copy(pin + m * proof_stride, public_inputs + copied * in_row, m * in_row);
      auto tc = now();
      t_wait += ms(ta, tb); t_copy += ms(tb, tc);
      HIPCK(hipMemcpyAsync(d->st_proofs + copied * proof_stride, pin, m * proof_stride, hipMemcpyHostToDevice, ring.copy));
      if (in_row) HIPCK(hipMemcpyAsync(d->st_inputs + copied * in_row, pin + m * proof_stride, m * in_row, hipMemcpyHostToDevice, ring.copy));
      if ((rc = ring.commit())) return rc;
      copied += m;
    }
    if (ring.last()) HIPCK(hipStreamWaitEvent(ring.compute, ring.last(), 0));
    auto td = now();
    const Sp1Src staged = sp1 ? Sp1Src{d->st_vkh + (sp1->vkh_stride ? computed * 32 : 0), (size_t)(sp1->vkh_stride ? 32 : 0), d->st_pv, pv_total, sp1->off[0], (const uint64_t*)(uint8_t*)d->st_off + computed}
                              : Sp1Src{};
    rc = g16_enqueue(pvk, d, device, d->st_proofs + computed * proof_stride, proof_stride, d->st_inputs + computed * in_row, n_public, c_end - computed,
                     d->st_status + computed, ring.compute, flags, use_rlc, sp1 ? &staged : nullptr);
    if (rc) return ring.drain(rc);
    t_enq += ms(td, now());
    computed = c_end;
    c_end = n - c_end < hchunk ? n : c_end + hchunk;
  }
  const auto t_enqueued = now();
  HIPCK(hipMemcpyAsync(status, d->st_status, n, hipMemcpyDeviceToHost, ring.compute));
  HIPCK(hipStreamSynchronize(ring.compute));
  if (timing) fprintf(stderr, "host-buffer batch %zu: pieces of %zu proofs; host copies %.2f ms, ring waits %.2f ms, kernel enqueue %.2f ms, all enqueued after %.2f ms, done after %.2f ms\n",
                      n, piece, t_copy, t_wait, t_enq, ms(t_begin, t_enqueued), ms(t_begin, now()));
  return BN254_OK;
}
int g16_sp1_host(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const Sp1Src& s, size_t n, uint8_t* status, int device, unsigned flags) {
  return g16_host_batch(pvk, proofs, proof_stride, nullptr, 0, n, status, device, flags, &s);
}

extern "C" {

int bn254_groth16_verify_batch(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                               size_t n_public, size_t n, uint8_t* status, int device, unsigned flags) {
  int rc = check_batch_args(false, pvk, proofs, proof_stride, public_inputs, n_public, n, status, flags);
  if (rc || n == 0) return rc;
  return g16_host_batch(pvk, proofs, proof_stride, public_inputs, n_public, n, status, device, flags, nullptr);
}

int bn254_groth16_verify_batch_multi(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                                     size_t n_public, size_t n, uint8_t* status, uint64_t device_mask, unsigned flags) {
  int prc = check_batch_args(false, pvk, proofs, proof_stride, public_inputs, n_public, n, status, flags);
  if (prc) return prc;
  if (!device_mask) return set_err(BN254_E_BAD_ARG, "bad argument");
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return set_err(BN254_E_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  int devs[64], nsh = 0; size_t los[64], cnts[64];
  if ((prc = bn254_shard_plan(n, device_mask, cnt, devs, los, cnts, &nsh))) return prc;
  const size_t w = (size_t)nsh;
  if (w == 1) return bn254_groth16_verify_batch(pvk, proofs, proof_stride, public_inputs, n_public, n, status, devs[0], flags);
  // one host thread per device drives its shard
  std::vector<int> rcs(w, BN254_OK); std::vector<std::string> errs(w);
  std::vector<std::thread> th;
  for (size_t r = 0; r < w; r++) {
    const size_t lo = los[r], cntp = cnts[r];
    th.emplace_back([&, r, lo, cntp]() {
      if (!cntp) return;
      rcs[r] = bn254_groth16_verify_batch(pvk, proofs + lo * proof_stride, proof_stride, public_inputs ? public_inputs + lo * n_public * 32 : nullptr, n_public, cntp,
                                          status + lo, devs[r], flags);
      if (rcs[r]) errs[r] = g_err;   // thread-local in the worker
    });
  }
  for (auto& t : th) t.join();
  for (size_t r = 0; r < w; r++) if (rcs[r]) return set_err(rcs[r], "device " + std::to_string(devs[r]) + ": " + errs[r]);
  return BN254_OK;
}

// load_groth16_proof_from_bytes (groth16/converter.rs:14-26) on the host, for the one case in which no kernel can run: a single proof against key bytes that do not
// load.  A, B, C in this order; per point: every coordinate < p (Field(NotMember)), the curve equation (Group(NotOnCurve)), and for B the r-torsion (Group(NotInSubgroup)).
static uint8_t g16_proof_loader_status(const uint8_t* p /* 256 bytes */) {
  auto g1 = [](const uint8_t* b) -> uint8_t {
    if (!be_lt_p(b) || !be_lt_p(b + 32)) return BN254_ERR_NOT_MEMBER;
    G1Aff a; a.x = fp_from_be(b); a.y = fp_from_be(b + 32);
    return g1_on_curve(a) ? BN254_ACCEPT : BN254_ERR_NOT_ON_CURVE;
  };
  uint8_t st = g1(p);
  if (st != BN254_ACCEPT) return st;
  for (int i = 0; i < 4; i++) if (!be_lt_p(p + 64 + 32 * i)) return BN254_ERR_NOT_MEMBER;
  G2Aff b; b.x.c1 = fp_from_be(p + 64); b.x.c0 = fp_from_be(p + 96); b.y.c1 = fp_from_be(p + 128); b.y.c0 = fp_from_be(p + 160);
  if (!g2_on_curve(b)) return BN254_ERR_NOT_ON_CURVE;
  if (!g2_in_subgroup(b)) return BN254_ERR_NOT_IN_SUBGROUP;
  return g1(p + 192);
}
int bn254_groth16_verify(const uint8_t* proof, size_t proof_len, const uint8_t* vk, size_t vk_len, const uint8_t* public_inputs,
                         size_t n_public, unsigned mode, uint8_t* status) {
  if (!proof || !vk || !status || mode > 1) return set_err(BN254_E_BAD_ARG, "bad argument");
  // reference order: the proof is loaded (and its errors surface) before the key (lib.rs:45-46).  A short proof buffer is a
  // slice-index panic there.
  if (proof_len < 256) { *status = BN254_ERR_MALFORMED; return BN254_OK; }
  // the reference parses the key on every call (lib.rs:46); here the prepared form of the last few keys is kept (exact byte match), so a
  // caller that verifies one proof at a time against the same key pays the preparation (9 ms of an 11 ms call) once
  std::shared_ptr<bn254_g16_pvk> pvk = g16_key_cache().find(vk, vk_len, mode);
  if (!pvk) {
    bn254_g16_pvk* raw = nullptr;
    int rc = bn254_groth16_vk_prepare(vk, vk_len, mode, &raw);
    if (rc == BN254_E_VK) {
      // the key does not load (lib.rs:46 panics) -- but the proof was loaded first (lib.rs:45), so its loader error wins.  Nothing can be launched without a key: the
      // loader's checks (< p, curve equation, r-torsion of B; groth16/converter.rs:14-26) run here on the host, once, for this one proof
      const uint8_t ps = g16_proof_loader_status(proof);
      *status = ps == BN254_ACCEPT ? (uint8_t)BN254_ERR_MALFORMED : ps;
      return BN254_OK;
    }
    if (rc) return rc;
    pvk = g16_key_cache().insert(vk, vk_len, mode, raw);
  }
  return bn254_groth16_verify_batch(pvk.get(), proof, proof_len, public_inputs, n_public, 1, status, 0, 0);
}

int bn254_groth16_proof_write_raw(const uint8_t a[64], const uint8_t b[128], const uint8_t c[64], uint8_t out[BN254_GROTH16_RAW_PROOF_LEN]) {
  if (!a || !b || !c || !out) return set_err(BN254_E_BAD_ARG, "bad argument");
  memcpy(out, a, 64); memcpy(out + 64, b, 128); memcpy(out + 192, c, 64);
  memset(out + 256, 0, BN254_GROTH16_RAW_PROOF_LEN - 256);   // u32 nbCommitments = 0, then the 64-byte commitment PoK (zero)
  return BN254_OK;
}

}  // extern "C"
