// bn254_capi_plonk_keys.hip -- PlonK batches over many verifying keys in one call (include/bn254_verify.h, "PlonK batches over many keys"): the per (key list,
// device) state -- the descriptors of the members' own device tables, a pool of pass contexts, the buffers of a call -- the plan over slots, what a pass over slots
// has around the one pass of bn254_capi_plonk.hip (plonk_pass: gather before, scatter after, the counters) and the three entries.  The grouping is Groth16's
// (bn254_keys.h, k_keys_count / _scan / _place) and so is the cache of the sets (bn254_capi_internal.h, KeySetCache); the kernels of a pass are the `_keys` twins of
// the single-key ones, beside them in bn254_k_plonk.hip, bn254_k_msm.hip, bn254_k_miller.hip, and the gather / scatter pair in bn254_k_keys.hip.
#include "bn254_capi_internal.h"
#include "bn254_keys.h"

using bn254::PlonkKeyDesc;

#define PLONK_KEYS_HOST_PIECE ((size_t)16 << 20)
#define PLONK_KEYS_MAX_PUBLIC ((size_t)1 << 20)     // a key that claims more inputs than this is not one a row can be passed for

// The knob of a pass's per-proof pairing check (bn254_set_plonk_keys_params; BN254_PLONK_KEYS_COOP_MAX gives the initial value once, at load time): passes of up to
// this many slots take the cooperative form (k_coop12_miller_fixed_keys), larger ones the lane form; 0: always the lane form.  BN254_COOP=0 switches it off
#define PLONK_KEYS_COOP_MAX_DEFAULT COOP12_MAX_PROOFS_FIXED
static long pk_coop_clamp(long v) { return v > (long)COOP12_MAX_PROOFS_FIXED ? (long)COOP12_MAX_PROOFS_FIXED : v; }
static std::atomic<long> g_pk_coop_max{[] { long v = env_long("BN254_PLONK_KEYS_COOP_MAX", (long)PLONK_KEYS_COOP_MAX_DEFAULT); return v < 0 ? (long)PLONK_KEYS_COOP_MAX_DEFAULT : pk_coop_clamp(v); }()};
bool plonk_keys_coop_form(size_t n) { return bn254::knob_coop_on() && n <= (size_t)g_pk_coop_max.load(std::memory_order_relaxed); }

namespace {

inline size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }

// ---- the plan of a batch over S slots: plonk_plan_for over slots, cuts on granule boundaries -------------------------------------------------------------
struct PkPlan { int workers; size_t per, pass; };
PkPlan pk_plan(size_t slots) {
  PkPlan p; size_t per, pass;
  plonk_plan_for(slots, &p.workers, &per, &pass);
  p.per = up64(per); p.pass = up64(pass);      // a cut may fall inside a key's run, never inside a granule
  const int used = (int)((slots + p.per - 1) / p.per);
  if (used < p.workers) p.workers = used < 1 ? 1 : used;
  return p;
}
// What the contexts of a set must hold so that ANY batch of up to hi slots runs without growing them: the largest pass and the most workers of any slot count up to
// hi.  Within a segment of the plan (plonk_plan_breaks) neither the piece nor the worker count falls as the batch grows, so the ends of the segments are the candidates;
// a pass never exceeds min(slots, piece), rounded up to a granule.
void pk_capacity(size_t hi, size_t* pass_slots, int* workers) {
  size_t br[4], best = 0; int w = 1;
  const int nb = plonk_plan_breaks(br);
  auto at = [&](size_t s) {      // s: a slot count, a multiple of 64
    if (s < 64) return;
    int mw; const size_t piece = plonk_piece_for(s, &mw);
    const size_t v = s < piece ? s : piece;
    if (v > best) best = v;
    const PkPlan p = pk_plan(s);
    if (p.workers > w) w = p.workers;
  };
  at(up64(hi));
  for (int i = 0; i < nb; i++) if (br[i] < hi) at(br[i] & ~(size_t)63);      // the largest slot count of the segment
  *pass_slots = up64(best); *workers = w;
}
// the capacity plonk_ensure_ctx gives a context asked to hold `need` proofs
size_t pk_ctx_cap(size_t need) { return need < PLONK_MAX_LAUNCH ? (need + 255) / 256 * 256 : (size_t)PLONK_MAX_LAUNCH; }

// ---- what one call holds beside its contexts: the grouping of ITS batch and, for the host-buffer entry, the device copies of the caller's buffers -----------
struct PkCall {
  PinRing ring;                        // ring.compute: the call's stream (grouping, the copies of a host-buffer call)
  DevBuf<uint32_t> count, base, cursor, n_slots, slot_to_proof, granule_key;
  PinBuf<uint32_t> h_slots;
  DevBuf<uint8_t> st_proofs, st_inputs, st_status; DevBuf<uint32_t> st_index;
};
struct PkCtxExtra { DevBuf<uint8_t> recs, rows; };      // the records and input rows of a pass in slot order

struct PlonkKeySet {
  std::vector<const bn254_plonk_pvk*> list;   // the handles as passed (order matters: key_index refers to it)
  int device = 0;
  size_t max_public = 0;
  size_t staged_public = 0;                   // the most inputs any member stages in LDS (bn254_launch_plonk_stage1_keys); with the descriptors, at the first use
  std::mutex mu;                              // the first use (descriptors) and the list of free call buffers
  bool ready = false;
  DevBuf<PlonkKeyDesc> desc;
  const int32_t* one = nullptr;               // 1 in GT: member 0's copy
  // the contexts of the set's passes, leased as a key's are (PlonkLease): of a PlonkDev only ctx / pool_mu / pool_cv / busy are used here
  PlonkDev pool;
  PkCtxExtra extra[PLONK_WORKERS];
  std::vector<std::unique_ptr<PkCall>> free_calls;
  // bn254_plonk_keys_state: passes that ran the joint check | groups they checked | groups that failed | passes whose per-proof check ran in the cooperative form
  std::atomic<uint64_t> stat[4] = {};
  ~PlonkKeySet() {
    if (!ready && free_calls.empty()) return;
    if (hipSetDevice(device) == hipSuccess) (void)hipDeviceSynchronize();      // the members below release what they own on a device that is current and idle
  }
};
struct CallLease {    // a call's buffers: taken from the set's free list (or new), given back when the call returns
  PlonkKeySet& s; std::unique_ptr<PkCall> c;
  explicit CallLease(PlonkKeySet& s_) : s(s_) {
    std::lock_guard<std::mutex> lk(s.mu);
    if (!s.free_calls.empty()) { c = std::move(s.free_calls.back()); s.free_calls.pop_back(); }
    else c.reset(new PkCall());
  }
  ~CallLease() { std::lock_guard<std::mutex> lk(s.mu); s.free_calls.push_back(std::move(c)); }
};

KeySetCache<PlonkKeySet, bn254_plonk_pvk>& pk_cache() { static auto* c = new KeySetCache<PlonkKeySet, bn254_plonk_pvk>(); return *c; }

// ---- arguments ---------------------------------------------------------------------------------------------------------------------------------------------------
int pk_check_list(const bn254_plonk_pvk* const* pvks, size_t n_keys, size_t* max_public) {
  if (!pvks || n_keys == 0) return set_err(BN254_E_BAD_ARG, "bad argument: empty key list");
  if (n_keys > (size_t)PLONK_KEYS_MAX_KEYS) {
    set_diag("a PlonK key list holds at most " + std::to_string(PLONK_KEYS_MAX_KEYS) + " entries (got " + std::to_string(n_keys) + ")");
    return set_err(BN254_E_BAD_ARG, "key list too long");
  }
  size_t mx = 0;
  for (size_t k = 0; k < n_keys; k++) {
    if (!pvks[k]) return set_err(BN254_E_BAD_ARG, "bad argument: null key in the list");
    if (pvks[k]->key.n_qcp != pvks[0]->key.n_qcp) {
      set_diag("entry " + std::to_string(k) + " of the key list has " + std::to_string(pvks[k]->key.n_qcp) + " BSB22 commitments, entry 0 has " + std::to_string(pvks[0]->key.n_qcp) +
               ": all keys of a list must have the same number (it fixes the term counts and the MSM plans of a pass); one list per commitment count");
      return set_err(BN254_E_BAD_ARG, "the keys of the list differ in their number of BSB22 commitments");
    }
    const uint64_t p = pvks[k]->key.nb_public;
    if (p > PLONK_KEYS_MAX_PUBLIC) return set_err(BN254_E_BAD_ARG, "a key of the list claims more than 2^20 public inputs");
    if ((size_t)p > mx) mx = (size_t)p;
  }
  *max_public = mx;
  return BN254_OK;
}
size_t pk_min_stride(const bn254_plonk_pvk* pvk) { return 808 + 96 * (size_t)pvk->key.n_qcp; }
int pk_check_args(const bn254_plonk_pvk* const* pvks, size_t n_keys, const void* key_index, const void* proofs, size_t proof_stride, const void* inputs, size_t input_stride,
                  size_t n, const void* status, unsigned flags, size_t* max_public) {
  int rc = pk_check_list(pvks, n_keys, max_public);
  if (rc) return rc;
  if (flags & ~(unsigned)BN254_FLAG_RLC) return set_err(BN254_E_BAD_ARG, "unknown flag (the PlonK batch entries know BN254_FLAG_RLC)");
  if (n && (!key_index || !proofs || !status)) return set_err(BN254_E_BAD_ARG, "bad argument: null pointer");
  if (proof_stride < pk_min_stride(pvks[0])) return set_err(BN254_E_BAD_ARG, "proof_stride is smaller than a proof of these keys (808 + 96 per BSB22 commitment)");
  if (input_stride < 32 * *max_public) return set_err(BN254_E_BAD_ARG, "input_stride is smaller than the inputs of the widest key of the list (32 bytes each)");
  if (n && *max_public && !inputs) return set_err(BN254_E_BAD_ARG, "bad argument: null public inputs");
  if (n && (proof_stride > SIZE_MAX / n || (input_stride && input_stride > SIZE_MAX / n) || bn254::keys_slot_bound(n, n_keys) > 0xffff0000ull))
    return set_err(BN254_E_BAD_ARG, "batch too large: slots and rows are addressed with 32 / 64 bits");
  return BN254_OK;
}

// ---- device state ----------------------------------------------------------------------------------------------------------------------------------------------
// caller holds s.mu.  First use: every distinct member's own device state (plonk_ensure_dev: window tables, line tables, the parsed key, its self-test) and the
// descriptors that point into it.
int pk_ensure_set(PlonkKeySet& s) {
  if (s.ready) return selftest_gate(s.device);      // (the device passed its self-test before the set became ready: this only reads the recorded state)
  int rc = check_device(s.device);
  if (rc || (rc = selftest_gate(s.device))) return rc;
  std::vector<const bn254_plonk_pvk*> order;
  for (auto p : s.list) if (std::find(order.begin(), order.end(), p) == order.end()) order.push_back(p);
  // the window tables still to build must fit beside their construction scratch and leave room for contexts
  size_t table_bytes = 0;
  for (auto p : order) {
    std::lock_guard<std::mutex> lk(p->mu);
    auto it = p->dev.find(s.device);
    if (it == p->dev.end() || !it->second.ready) table_bytes += (p->fixed_pts.size() / (2 * BN_NL)) * (size_t)MSM_FW_WINDOWS * MSM_FW_ENTRIES * MSM_ENTRY_DWORDS * sizeof(int32_t);
  }
  if (table_bytes) {
    size_t free_b = 0, total_b = 0;
    HIPCK(hipMemGetInfo(&free_b, &total_b));
    if (table_bytes + ((size_t)512 << 20) > free_b)
      return set_err(BN254_E_NOMEM, "the window tables of the list's keys (" + std::to_string(table_bytes >> 20) + " MB still to build, 13 MB per key point) do not fit the device's free memory (" +
                                        std::to_string(free_b >> 20) + " MB)");
  }
  std::vector<PlonkKeyDesc> desc(s.list.size());
  for (size_t k = 0; k < s.list.size(); k++) {
    const bn254_plonk_pvk* p = s.list[k];
    const size_t pub = (size_t)p->key.nb_public;
    if (pub * 32 <= 256 && pub > s.staged_public) s.staged_public = pub;
    PlonkDev* d;
    {
      std::lock_guard<std::mutex> lk(p->mu);
      if ((rc = plonk_ensure_dev(p, s.device, &d))) return rc;
    }
    desc[k].key = (const uint8_t*)d->d_key; desc[k].fixed_tabs = d->fixed_tabs; desc[k].tab0 = d->tab0; desc[k].tab1 = d->tab1;
    desc[k].n_public = (uint32_t)p->key.nb_public; desc[k].pad_ = 0;
    if (k == 0) s.one = d->one;
  }
  if ((rc = upload(s.desc, desc))) return rc;
  s.ready = true;
  return BN254_OK;
}
// the buffers of a call over n proofs; host: also the device copies of the caller's buffers and the pinned ring they travel through
int pk_ensure_call(const PlonkKeySet& s, PkCall& c, size_t n, bool host, size_t proof_stride, size_t input_stride) {
  const int oom = BN254_E_NOMEM;
  const size_t n_keys = s.list.size(), bound = (size_t)bn254::keys_slot_bound(n, n_keys);
  int rc;
  if ((rc = c.ring.ensure(host ? PLONK_KEYS_HOST_PIECE : 0))) return rc;
  if ((rc = c.count.ensure(n_keys, oom)) || (rc = c.base.ensure(n_keys, oom)) || (rc = c.cursor.ensure(n_keys, oom)) || (rc = c.n_slots.ensure(1, oom)) ||
      (rc = c.slot_to_proof.ensure(bound, oom)) || (rc = c.granule_key.ensure(bound / G16_KEYS_GRANULE + 1, oom)) || (rc = c.h_slots.ensure(1)))
    return rc;
  if (host) {
    const size_t in_bytes = s.max_public ? n * input_stride : 0;
    if ((rc = c.st_proofs.ensure(n * proof_stride, oom)) || (rc = c.st_inputs.ensure(in_bytes ? in_bytes : 32, oom)) || (rc = c.st_index.ensure(n, oom)) || (rc = c.st_status.ensure(n, oom)))
      return rc;
  }
  return BN254_OK;
}
size_t pk_rec_bytes(size_t proof_stride) { return proof_stride < 1664 ? proof_stride : 1664; }      // what the stage kernels read of a record (PL_STAGE_MAX_PROOF)
// context w of a lease for passes of up to `slots` slots of records of this stride.  All members share the shapes that size a context: member 0 stands for them
int pk_ensure_ctx(PlonkKeySet& s, const PlonkLease& lease, int w, size_t slots, size_t proof_stride) {
  PlonkCtx& c = lease.ctx(w);
  int rc = plonk_ensure_ctx(s.list[0], c, slots, 0);
  if (rc) return rc;
  PkCtxExtra& x = s.extra[lease.idx[w]];
  const size_t rec_stride = (pk_rec_bytes(proof_stride) + 3) & ~(size_t)3;
  if ((rc = x.recs.ensure(c.cap * rec_stride, BN254_E_NOMEM)) || (rc = x.rows.ensure(c.cap * 32 * s.max_public, BN254_E_NOMEM))) return rc;
  // BN254_FLAG_RLC: one group per granule of the capacity, points and status byte, and the failure count with its pinned copy
  if (c.grp_ws.cap() < c.cap / 64 * (size_t)(G16_WS_BYTES_PER_PROOF / 4) || c.grp_status.cap() < c.cap / 64 || !c.d_fail || !c.h_fail)
    return set_err(BN254_E_HIP, "PlonK key-set context without the group buffers of its capacity (internal sizing error)");
  return BN254_OK;
}

// ---- one pass: slots [s0, s0 + m) of the call's grouping on context c: gather, the pass (plonk_pass), scatter ----------------------------------------------------
// the front of a pass: its records and rows gathered in slot order on c.stream; *t / *in: what the pass then runs on
int pk_gather_pass(PlonkKeySet& s, PlonkCtx& c, PkCtxExtra& x, const PkCall& call, size_t s0, size_t m, const uint8_t* d_proofs, size_t proof_stride, const uint8_t* d_inputs,
                   size_t input_stride, size_t n, PlonkTables* t, PlonkPassIn* in) {
  HIPCK(hipSetDevice(s.device));
  const uint32_t n_keys = (uint32_t)s.list.size();
  const size_t rec_bytes = pk_rec_bytes(proof_stride), rec_stride = (rec_bytes + 3) & ~(size_t)3, row_stride = 32 * s.max_public;
  if (m > c.cap || m * rec_stride > x.recs.cap() || m * row_stride > x.rows.cap() || (m & 63)) return set_err(BN254_E_HIP, "PlonK key-set context smaller than the pass (internal sizing error)");
  const uint32_t* s2p = call.slot_to_proof + s0;
  const uint32_t* gk = call.granule_key + s0 / G16_KEYS_GRANULE;
  hipError_t e = bn254_launch_plonk_keys_gather(d_proofs, proof_stride, d_inputs, input_stride, (uint32_t)n, s2p, gk, s.desc, n_keys, (uint32_t)m, x.recs, (uint32_t)rec_stride,
                                                (uint32_t)rec_bytes, x.rows, (uint32_t)row_stride, c.stream);
  if (e != hipSuccess) return launch_err(e, "PlonK key-set gather");
  *t = PlonkTables{nullptr, s.desc, n_keys, gk, s.one};
  *in = PlonkPassIn{x.recs, rec_stride, row_stride ? (const uint8_t*)x.rows : nullptr, 0, proof_stride, row_stride, s.staged_public};
  return BN254_OK;
}
int pk_run_pass(PlonkKeySet& s, PlonkCtx& c, PkCtxExtra& x, const PkCall& call, size_t s0, size_t m, const uint8_t* d_proofs, size_t proof_stride, const uint8_t* d_inputs,
                size_t input_stride, size_t n, uint8_t* d_status, unsigned flags) {
  PlonkTables t; PlonkPassIn in;
  int rc = pk_gather_pass(s, c, x, call, s0, m, d_proofs, proof_stride, d_inputs, input_stride, n, &t, &in);
  if (rc) return rc;
  const uint32_t* s2p = call.slot_to_proof + s0;
  // all members share the shapes of a pass: member 0 stands for them
  PlonkPassReport rep;
  if ((rc = plonk_pass(s.list[0], t, in, c, m, flags, nullptr, &rep))) return rc;
  hipError_t e;
  if (rep.joint) { s.stat[0].fetch_add(1, std::memory_order_relaxed); s.stat[1].fetch_add(rep.groups, std::memory_order_relaxed); s.stat[2].fetch_add(rep.failed, std::memory_order_relaxed); }
  if (rep.exact && plonk_keys_coop_form(m)) s.stat[3].fetch_add(1, std::memory_order_relaxed);
  e = bn254_launch_plonk_keys_scatter(c.status, s2p, (uint32_t)m, (uint32_t)n, d_status, c.stream);
  if (e != hipSuccess) return launch_err(e, "PlonK key-set scatter");
  HIPCK(hipStreamSynchronize(c.stream));
  return BN254_OK;
}

// One batch on device buffers.  The grouping runs on the call's stream (after whatever that stream still copies); its slot count is read back -- 4 bytes, one wait: the
// entries are synchronous anyway -- and the passes of the plan over that many slots run on leased contexts, one host thread per worker.
int pk_batch(PlonkKeySet& s, PkCall& call, const uint32_t* d_index, const uint8_t* d_proofs, size_t proof_stride, const uint8_t* d_inputs, size_t input_stride, size_t n,
             uint8_t* d_status, unsigned flags) {
  const uint32_t n_keys = (uint32_t)s.list.size();
  const size_t bound = (size_t)bn254::keys_slot_bound(n, n_keys);
  hipStream_t cs = call.ring.compute;
  hipError_t e = bn254_launch_keys_group(d_index, (uint32_t)n, n_keys, (uint32_t)bound, call.count, call.base, call.cursor, call.n_slots, call.slot_to_proof, call.granule_key, d_status, cs);
  if (e != hipSuccess) return launch_err(e, "grouping");
  HIPCK(hipMemcpyAsync(call.h_slots, call.n_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
  HIPCK(hipStreamSynchronize(cs));
  const size_t slots = *call.h_slots;
  if (slots > bound || (slots & 63)) return set_err(BN254_E_HIP, "grouping returned an impossible slot count");
  if (slots == 0) return BN254_OK;          // every index was outside the list: k_keys_place has answered MALFORMED for all
  const PkPlan plan = pk_plan(slots);
  PlonkLease lease(&s.pool, plan.workers);
  int rc;
  for (int w = 0; w < plan.workers; w++) if ((rc = pk_ensure_ctx(s, lease, w, plan.pass, proof_stride))) return rc;
  return plonk_run_workers(lease, plan.workers, plan.per, plan.pass, slots, [&](int w, size_t off, size_t m) {
    return pk_run_pass(s, lease.ctx(w), s.extra[lease.idx[w]], call, off, m, d_proofs, proof_stride, d_inputs, input_stride, n, d_status, flags);
  });
}

std::shared_ptr<PlonkKeySet> pk_get_ready(const bn254_plonk_pvk* const* pvks, size_t n_keys, int device, size_t max_public, int* rc) {
  std::shared_ptr<PlonkKeySet> s = pk_cache().get(pvks, n_keys, device, max_public);
  std::lock_guard<std::mutex> lk(s->mu);
  *rc = pk_ensure_set(*s);
  return s;
}

}  // namespace

// bn254_plonk_vk_free: every cached set that contains the key goes
void plonk_keys_sets_drop(const bn254_plonk_pvk* member) { pk_cache().drop(member); }

// The value probe over a key list (bn254_dbg_plonk_stages_keys): the host entry's checks, the batch's buffers on the device, the grouping, and every slot gathered as
// ONE pass on one leased context -- then `body` instead of plonk_pass.  The pass is not cut: a probe batch is small, and the slot a proof is given is what its lambda
// and weight are drawn by
int plonk_keys_probe_pass(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                          size_t input_stride, size_t n, unsigned flags, int device, const std::function<int(const PlonkKeysProbePass&)>& body) {
  size_t max_public = 0;
  int rc = pk_check_args(pvks, n_keys, key_index, proofs, proof_stride, public_inputs, input_stride, n, proofs, flags, &max_public);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++)
    if (key_index[i] >= n_keys) return set_err(BN254_E_BAD_ARG, "key_index[" + std::to_string(i) + "] = " + std::to_string(key_index[i]) + " is outside the list of " + std::to_string(n_keys) + " keys");
  if ((rc = check_device(device))) return rc;
  std::shared_ptr<PlonkKeySet> s = pk_get_ready(pvks, n_keys, device, max_public, &rc);
  if (rc) return rc;
  CallLease cl(*s);
  PkCall& c = *cl.c;
  if ((rc = pk_ensure_call(*s, c, n, true, proof_stride, input_stride))) return rc;
  const size_t in_bytes = max_public ? n * input_stride : 0;
  HIPCK(hipMemcpy((uint32_t*)c.st_index, key_index, n * 4, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(c.st_proofs, proofs, n * proof_stride, hipMemcpyHostToDevice));
  if (in_bytes) HIPCK(hipMemcpy(c.st_inputs, public_inputs, in_bytes, hipMemcpyHostToDevice));
  const size_t bound = (size_t)bn254::keys_slot_bound(n, n_keys);
  hipStream_t cs = c.ring.compute;
  hipError_t e = bn254_launch_keys_group(c.st_index, (uint32_t)n, (uint32_t)n_keys, (uint32_t)bound, c.count, c.base, c.cursor, c.n_slots, c.slot_to_proof, c.granule_key, c.st_status, cs);
  if (e != hipSuccess) return launch_err(e, "grouping");
  HIPCK(hipMemcpyAsync(c.h_slots, c.n_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
  HIPCK(hipStreamSynchronize(cs));
  const size_t slots = *c.h_slots;
  if (slots == 0 || slots > bound || (slots & 63)) return set_err(BN254_E_HIP, "grouping returned an impossible slot count");
  PlonkLease lease(&s->pool, 1);
  if ((rc = pk_ensure_ctx(*s, lease, 0, slots, proof_stride))) return rc;
  PlonkCtx& ctx = lease.ctx(0);
  PlonkKeysProbePass p;
  p.shapes = s->list[0]; p.c = &ctx; p.slots = slots; p.slot_to_proof = c.slot_to_proof;
  rc = pk_gather_pass(*s, ctx, s->extra[lease.idx[0]], c, 0, slots, c.st_proofs, proof_stride, in_bytes ? (const uint8_t*)c.st_inputs : nullptr, input_stride, n, &p.t, &p.in);
  if (!rc) rc = body(p);
  if (rc) { const std::string keep = g_err; (void)hipStreamSynchronize(ctx.stream); return set_err(rc, keep); }      // nothing of the pass in flight when the lease ends
  HIPCK(hipStreamSynchronize(ctx.stream));
  return BN254_OK;
}

extern "C" {

int bn254_plonk_reserve_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, size_t n, size_t proof_stride, int device) {
  size_t max_public = 0;
  int rc = pk_check_list(pvks, n_keys, &max_public);
  if (rc) return rc;
  if (proof_stride < pk_min_stride(pvks[0])) return set_err(BN254_E_BAD_ARG, "proof_stride is smaller than a proof of these keys (808 + 96 per BSB22 commitment)");
  if (n == 0) n = 1;
  if (proof_stride > SIZE_MAX / n || bn254::keys_slot_bound(n, n_keys) > 0xffff0000ull) return set_err(BN254_E_BAD_ARG, "batch too large: slots and rows are addressed with 32 / 64 bits");
  if ((rc = check_device(device))) return rc;
  std::shared_ptr<PlonkKeySet> s = pk_get_ready(pvks, n_keys, device, max_public, &rc);
  if (rc) return rc;
  {
    CallLease cl(*s);
    if ((rc = pk_ensure_call(*s, *cl.c, n, true, proof_stride, 32 * max_public))) return rc;
  }
  size_t pass_slots; int workers;
  pk_capacity((size_t)bn254::keys_slot_bound(n, n_keys), &pass_slots, &workers);
  PlonkLease lease(&s->pool, workers);
  for (int w = 0; w < workers; w++) {
    if ((rc = pk_ensure_ctx(*s, lease, w, pass_slots, proof_stride))) return rc == BN254_E_HIP && g_err.find("out of memory") != std::string::npos ? set_err(BN254_E_NOMEM, g_err) : rc;
  }
  return BN254_OK;
}

int bn254_plonk_verify_batch_keys_device(const bn254_plonk_pvk* const* pvks, size_t n_keys, const void* d_key_index, const void* d_proofs, size_t proof_stride,
                                         const void* d_public_inputs, size_t input_stride, size_t n, void* d_status, int device, void* hip_stream, unsigned flags) {
  size_t max_public = 0;
  int rc = pk_check_args(pvks, n_keys, d_key_index, d_proofs, proof_stride, d_public_inputs, input_stride, n, d_status, flags, &max_public);
  if (rc || n == 0) return rc;
  if ((rc = check_device(device))) return rc;
  // the passes run on the set's own streams: whatever the caller's stream still has to do to the inputs comes first
  HIPCK(hipStreamSynchronize((hipStream_t)hip_stream));
  std::shared_ptr<PlonkKeySet> s = pk_get_ready(pvks, n_keys, device, max_public, &rc);
  if (rc) return rc;
  CallLease cl(*s);
  if ((rc = pk_ensure_call(*s, *cl.c, n, false, proof_stride, input_stride))) return rc;
  return pk_batch(*s, *cl.c, (const uint32_t*)d_key_index, (const uint8_t*)d_proofs, proof_stride, (const uint8_t*)d_public_inputs, input_stride, n, (uint8_t*)d_status, flags);
}

// Host buffers: the index is checked on the host first (the range check the device entry cannot make), then index, records and input rows go up through the call's
// ring of pinned pieces, the device entry's pipeline runs on the copies and the status bytes come back.
int bn254_plonk_verify_batch_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride,
                                  const uint8_t* public_inputs, size_t input_stride, size_t n, uint8_t* status, int device, unsigned flags) {
  size_t max_public = 0;
  int rc = pk_check_args(pvks, n_keys, key_index, proofs, proof_stride, public_inputs, input_stride, n, status, flags, &max_public);
  if (rc || n == 0) return rc;
  for (size_t i = 0; i < n; i++)
    if (key_index[i] >= n_keys) return set_err(BN254_E_BAD_ARG, "key_index[" + std::to_string(i) + "] = " + std::to_string(key_index[i]) + " is outside the list of " + std::to_string(n_keys) + " keys");
  if ((rc = check_device(device))) return rc;
  std::shared_ptr<PlonkKeySet> s = pk_get_ready(pvks, n_keys, device, max_public, &rc);
  if (rc) return rc;
  CallLease cl(*s);
  PkCall& c = *cl.c;
  if ((rc = pk_ensure_call(*s, c, n, true, proof_stride, input_stride))) return rc;
  const size_t in_bytes = max_public ? n * input_stride : 0;
  PinRing& ring = c.ring;
  ring.begin();
  auto push = [&](uint8_t* dst, const uint8_t* src, size_t len) { return ring.push(dst, len, [src](uint8_t* q, size_t from, size_t k) { parallel_copy(q, src + from, k); }); };
  if ((rc = push((uint8_t*)(uint32_t*)c.st_index, (const uint8_t*)key_index, n * 4)) || (rc = push(c.st_proofs, proofs, n * proof_stride)) ||
      (in_bytes && (rc = push(c.st_inputs, public_inputs, in_bytes))))
    return ring.drain(rc);
  if (ring.last()) HIPCK(hipStreamWaitEvent(ring.compute, ring.last(), 0));
  if ((rc = pk_batch(*s, c, c.st_index, c.st_proofs, proof_stride, in_bytes ? (const uint8_t*)c.st_inputs : nullptr, input_stride, n, c.st_status, flags))) return ring.drain(rc);
  HIPCK(hipMemcpyAsync(status, c.st_status, n, hipMemcpyDeviceToHost, ring.compute));
  HIPCK(hipStreamSynchronize(ring.compute));
  return BN254_OK;
}

void bn254_set_plonk_keys_params(long coop_max) {
  if (coop_max >= 0) g_pk_coop_max.store(pk_coop_clamp(coop_max));
}
// the two knobs a batch over a list follows, as they are now (the setters clamp): out[0] coop_max, out[1] the pass size from which BN254_FLAG_RLC is honoured
int bn254_dbg_plonk_keys_knobs(long out[2]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  out[0] = g_pk_coop_max.load(); out[1] = (long)plonk_rlc_min();
  return BN254_OK;
}
int bn254_plonk_keys_state(const bn254_plonk_pvk* const* pvks, size_t n_keys, int device, uint64_t out[4]) {
  if (!pvks || !out || n_keys == 0) return set_err(BN254_E_BAD_ARG, "bad argument");
  for (size_t k = 0; k < n_keys; k++) if (!pvks[k]) return set_err(BN254_E_BAD_ARG, "bad argument: null key in the list");
  std::shared_ptr<PlonkKeySet> s = pk_cache().find(pvks, n_keys, device);
  if (!s) return set_err(BN254_E_BAD_ARG, "no cached state for this key list on this device (no batch or reservation yet, or it was evicted)");
  for (int i = 0; i < 4; i++) out[i] = s->stat[i].load(std::memory_order_relaxed);
  return BN254_OK;
}
// k_coop12_miller_fixed_keys in store mode on the line tables of prepared PlonK keys, shaped as bn254_dbg_coop12_miller_fixed: item i belongs to entry
// key_words[i >> key_shift] of the list; out_gt: the final-exponentiated product of its two pairings, 384 bytes per item
int bn254_dbg_coop12_miller_fixed_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_words, unsigned key_shift, const uint8_t* g1_0, const uint8_t* g1_1,
                                       const uint8_t* identity, uint8_t* out_gt, size_t n, int device) {
  if (!pvks || !key_words || !g1_0 || !g1_1 || !out_gt || n == 0 || key_shift > 31) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > bn254_coop_max_proofs_fixed()) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  size_t max_public = 0;
  int rc = pk_check_list(pvks, n_keys, &max_public);
  if (rc) return rc;
  if ((rc = check_device(device))) return rc;
  std::shared_ptr<PlonkKeySet> s = pk_get_ready(pvks, n_keys, device, max_public, &rc);      // the members' tables on the device, the descriptors
  if (rc) return rc;
  const size_t n_words = ((n - 1) >> key_shift) + 1;
  DevBuf<int32_t> ws; DevBuf<uint8_t> st_d, in, out; DevBuf<uint32_t> kw;
  std::vector<uint8_t> st(n);
  for (size_t i = 0; i < n; i++) st[i] = (uint8_t)(BN254_ST_PENDING | (identity && (identity[i] & 1) ? BN254_ST_LINF : 0) | (identity && (identity[i] & 2) ? BN254_ST_LINF2 : 0));
  if ((rc = ws.ensure(n * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = st_d.ensure(n)) || (rc = in.ensure(128 * n)) || (rc = out.ensure(384 * n)) || (rc = kw.ensure(n_words))) return rc;
  HIPCK(hipMemsetAsync(ws, 0, n * (size_t)G16_WS_BYTES_PER_PROOF, nullptr));
  HIPCK(hipMemcpy(in, g1_0, 64 * n, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(in + 64 * n, g1_1, 64 * n, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(kw, key_words, n_words * sizeof(uint32_t), hipMemcpyHostToDevice));
  hipError_t e = bn254_launch_dbg_load(ws, n, st_d, (int)VE_LX_ELEM, in, 4, nullptr);
  if (e == hipSuccess) e = bn254_launch_dbg_load(ws, n, st_d, (int)VE_CX_ELEM, in + 64 * n, 4, nullptr);
  if (e != hipSuccess) return launch_err(e, "probe");
  HIPCK(hipMemcpy(st_d, st.data(), n, hipMemcpyHostToDevice));      // after the loads (same stream): they set PENDING alone
  // the arguments of the product's cooperative calls, without the target
  e = bn254_coop12_miller_fixed_keys(ws, st_d, n, kw, key_shift, s->desc, (uint32_t)n_keys, nullptr, 0, nullptr);
  if (e == hipSuccess) e = bn254_launch_dbg_store(ws, n, (int)VE_S0, out, 0, nullptr);
  if (e != hipSuccess) return launch_err(e, "probe");
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(out_gt, out, 384 * n, hipMemcpyDeviceToHost));
  return BN254_OK;
}

// The plan of a batch, for the tests (host arithmetic only): n proofs over n_keys entries whose grouping came to `slots` slots, under the current knobs.
// ctx_capacity: the slots a context holds after bn254_plonk_reserve_keys for (n, n_keys); pass_first: the first slot of every pass, worker by worker (up to cap).
int bn254_dbg_plonk_keys_plan(size_t n, size_t n_keys, size_t slots, size_t* slot_bound, int* workers, size_t* per_worker, size_t* per_pass, size_t* ctx_capacity,
                              size_t* pass_first, size_t cap, size_t* n_passes) {
  if (!slot_bound || !workers || !per_worker || !per_pass || !ctx_capacity || !n_passes || (cap && !pass_first) || n == 0 || n_keys == 0 || n_keys > PLONK_KEYS_MAX_KEYS ||
      bn254::keys_slot_bound(n, n_keys) > 0xffff0000ull)
    return set_err(BN254_E_BAD_ARG, "bad argument");
  const size_t bound = (size_t)bn254::keys_slot_bound(n, n_keys);
  if (slots == 0 || slots > bound || (slots & 63)) return set_err(BN254_E_BAD_ARG, "slots must be a multiple of 64 between 64 and the slot bound");
  const PkPlan p = pk_plan(slots);
  size_t pass_slots; int w_res;
  pk_capacity(bound, &pass_slots, &w_res);
  *slot_bound = bound; *workers = p.workers; *per_worker = p.per; *per_pass = p.pass; *ctx_capacity = pk_ctx_cap(pass_slots);
  size_t k = 0;
  for (int w = 0; w < p.workers; w++) {
    const size_t lo = (size_t)w * p.per, hi = lo + p.per < slots ? lo + p.per : slots;
    for (size_t off = lo; off < hi; off += p.pass) { if (k < cap) pass_first[k] = off; k++; }
  }
  *n_passes = k;
  return BN254_OK;
}

}  // extern "C"
