// bn254_capi_keys.hip -- Groth16 batches over many verifying keys in one call (include/bn254_verify.h, "Batches over many keys"): the per (key list, device) state --
// descriptors, the keys' line tables, byte-window tables of all their K points in one allocation, the slot workspace -- and the three entries (the cache of the sets: bn254_capi_internal.h, KeySetCache).
// The kernels are in bn254_k_keys.hip / bn254_k_miller.hip (grouped form) and bn254_coop12.hip (direct form), the grouping arithmetic in bn254_keys.h, the choice
// between the forms in bn254_g16_plan.h.
#include "bn254_capi_internal.h"
#include "bn254_keys.h"

#include "bn254_vm.h"

using bn254::G16KeyDesc;

// The knob of the plan (bn254_set_keys_params; BN254_KEYS_COOP_MAX gives the initial value once, at load time): batches of up to this many proofs take the direct form
// (bn254_g16_plan.h::g16_keys_form).  A build without a device compiler (tests/hostsan) starts at 0 whatever the environment says: the grouped form at every size,
// until a harness that brings a stand-in for the direct launcher turns the knob.
static long keys_coop_clamp(long v) { return v > (long)COOP12_MAX_PROOFS ? (long)COOP12_MAX_PROOFS : v; }
#if defined(__HIPCC__)
static std::atomic<long> g_keys_coop_max{[] { long v = env_long("BN254_KEYS_COOP_MAX", (long)G16_KEYS_COOP_MAX_DEFAULT); return v < 0 ? (long)G16_KEYS_COOP_MAX_DEFAULT : keys_coop_clamp(v); }()};
#else
static std::atomic<long> g_keys_coop_max{0};
#endif
static int keys_form(size_t n) { return bn254::g16_keys_form(n, (size_t)g_keys_coop_max.load(std::memory_order_relaxed), bn254::knob_coop_on()); }

// A set does NOT make its members' own per-device state ready: ensure_dev builds a key's 13-bit window tables (13 MB per K point, bn254_fw.h), and a key that is only
// used through sets must never cost that.  The set keeps, per DISTINCT handle of the list (a handle may occur many times): both line tables, K[0] and e(alpha, beta)
// from the key's host half (KEYS_BLOB_DWORDS dwords, 38.5 KB) and byte-window tables of K[1..] (bn254_k_comb.hip form 1: 32 x 255 entries of 80 bytes = 652 800 bytes
// per point), all keys in one allocation each.
#define KEYS_BLOB_DWORDS ((size_t)2 * BN_ATE_STEPS * FIXED_LINE_DWORDS + 2 * BN_NL + 12 * BN_NL)
#define KEYS_TABLE_BYTES_PER_POINT ((size_t)32 * 255 * MSM_ENTRY_DWORDS * 4)
#define KEYS_HOST_PIECE ((size_t)16 << 20)

namespace {

struct KeySet {
  std::vector<const bn254_g16_pvk*> list;   // the handles as passed (order matters: key_index refers to it)
  int device = 0;
  size_t max_public = 0;
  std::mutex mu;                            // everything below: uploads, (re)allocation and the enqueue of a batch
  bool ready = false;
  DevBuf<int32_t> blob, msm; DevBuf<G16KeyDesc> desc;
  // what a reservation of n proofs sizes (ensure_set): the slot workspace (one chunk), the grouping buffers over keys_slot_bound(n, n_keys) slots
  size_t cap_n = 0, slot_cap = 0;
  DevBuf<int32_t> ws;
  size_t ws_slots() const { return ws.cap() / (size_t)(G16_WS_BYTES_PER_PROOF / 4); }
  DevBuf<uint32_t> count, base, cursor, n_slots, slot_to_proof, granule_key;
  DevBuf<uint8_t> slot_status;
  DevBuf<uint8_t> cmp; size_t cmp_cap = 0;                          // BN254_FLAG_COMPRESSED_PROOFS: raw records of the whole batch, then one pre-status byte per proof
  Stream aux; Event fork_ev, join_ev, busy_ev; bool busy_valid = false;
  int last_form = -1;                       // form of the last batch enqueued (bn254_dbg_g16_keys_last_form)
  // host-buffer entry: device copies of the caller's buffers, the pinned ring they travel through with its streams
  DevBuf<uint8_t> st_proofs, st_inputs, st_index, st_status;
  PinRing ring;
  // the members release what they own; the set's device is made current and idle first
  ~KeySet() {
    if (!ready && !ws && !blob) return;
    if (hipSetDevice(device) == hipSuccess) (void)hipDeviceSynchronize();
  }
};

KeySetCache<KeySet, bn254_g16_pvk>& set_cache() { static auto* c = new KeySetCache<KeySet, bn254_g16_pvk>(); return *c; }      // bn254_capi_internal.h

// caller holds s.mu.  First use: descriptors, line tables and byte-window tables of the distinct keys.  Then the buffers of a batch of n proofs (with
// BN254_FLAG_COMPRESSED_PROOFS in flags: its decompression scratch too).  Device memory that runs out here is BN254_E_NOMEM, as for tables that do not fit.
int ensure_set(KeySet& s, size_t n, unsigned flags) {
  const int oom = BN254_E_NOMEM;
  int rc = check_device(s.device);
  if (rc || (rc = selftest_gate(s.device))) return rc;
  const size_t n_keys = s.list.size();
  if (!s.ready) {
    std::map<const bn254_g16_pvk*, size_t> uniq;        // handle -> its number among the distinct ones
    std::vector<const bn254_g16_pvk*> order;
    for (auto p : s.list) if (uniq.emplace(p, order.size()).second) order.push_back(p);
    std::vector<size_t> first_point(order.size());
    std::vector<int32_t> pts, blob(order.size() * KEYS_BLOB_DWORDS);
    for (size_t u = 0; u < order.size(); u++) {
      const G16Prepared& h = order[u]->host;
      first_point[u] = pts.size() / (2 * BN_NL);
      pts.insert(pts.end(), h.kpts.begin(), h.kpts.end());
      if (h.kpts.size() != h.key_inputs() * 2 * BN_NL || h.gtab.size() != (size_t)BN_ATE_STEPS * FIXED_LINE_DWORDS || h.dtab.size() != h.gtab.size() || h.k0.size() != 2 * BN_NL ||
          h.target.size() != 12 * BN_NL)
        return set_err(BN254_E_BAD_ARG, "a key of the set does not carry its K points (prepared with host-built tables: BN254_TABLES_HOST)");
      int32_t* b = blob.data() + u * KEYS_BLOB_DWORDS;
      memcpy(b, h.gtab.data(), h.gtab.size() * 4); b += h.gtab.size();
      memcpy(b, h.dtab.data(), h.dtab.size() * 4); b += h.dtab.size();
      memcpy(b, h.k0.data(), h.k0.size() * 4); b += h.k0.size();
      memcpy(b, h.target.data(), h.target.size() * 4);
    }
    // the tables must fit beside the construction scratch (226 MB at most, bn254_capi.hip::build_tables_on_device) and leave room for a workspace
    size_t free_b = 0, total_b = 0;
    HIPCK(hipMemGetInfo(&free_b, &total_b));
    const size_t n_points = pts.size() / (2 * BN_NL), table_bytes = n_points * KEYS_TABLE_BYTES_PER_POINT;
    if (table_bytes + ((size_t)512 << 20) > free_b)
      return set_err(BN254_E_NOMEM, "the byte-window tables of the set (" + std::to_string(table_bytes >> 20) + " MB, 652 800 bytes per K point) do not fit the device's free memory (" +
                                        std::to_string(free_b >> 20) + " MB)");
    if ((rc = upload(s.blob, blob))) return rc;
    if (n_points && (rc = build_tables_on_device(1, pts, s.msm))) return rc;
    std::vector<G16KeyDesc> desc(n_keys);
    for (size_t k = 0; k < n_keys; k++) {
      const size_t u = uniq[s.list[k]];
      const G16Prepared& h = s.list[k]->host;
      const int32_t* b = s.blob + u * KEYS_BLOB_DWORDS;
      G16KeyDesc& d = desc[k];
      d.gtab = b; d.dtab = b + (size_t)BN_ATE_STEPS * FIXED_LINE_DWORDS; d.k0 = d.dtab + (size_t)BN_ATE_STEPS * FIXED_LINE_DWORDS; d.target = d.k0 + 2 * BN_NL;
      d.msm_tab = s.msm ? s.msm + first_point[u] * (KEYS_TABLE_BYTES_PER_POINT / 4) : s.blob;     // (never read for a key without inputs)
      d.n_public = (int32_t)h.key_inputs();
      d.inputs_match = h.n_k ? 1 : 0;
    }
    if ((rc = upload(s.desc, desc)) || (rc = s.busy_ev.ensure()) || (rc = s.fork_ev.ensure()) || (rc = s.join_ev.ensure()) || (rc = s.aux.ensure())) return rc;
    if ((rc = s.count.ensure(n_keys, oom)) || (rc = s.base.ensure(n_keys, oom)) || (rc = s.cursor.ensure(n_keys, oom)) || (rc = s.n_slots.ensure(1, oom))) return rc;
    // the direct form's kernel reads the step-kind table of the cooperative kernels, which is created on a device's first use: now, so that a batch only enqueues
    if (bn254_coop12_prepare() != hipSuccess) return set_err(oom, "out of device memory for the step table of the cooperative kernels");
    s.ready = true;
  }
  if (n > s.cap_n) {   // the workspace and the slot buffers are sized together: cap_n / slot_cap are what ALL of them hold, 0 while any of them is being replaced
    const size_t slot_cap = (size_t)bn254::keys_slot_bound(n, n_keys);
    const size_t ws_slots = bn254::g16_round256(slot_cap < (size_t)G16_MAX_BATCH ? slot_cap : (size_t)G16_MAX_BATCH);
    s.cap_n = s.slot_cap = 0;
    if ((rc = s.ws.ensure(ws_slots * (size_t)(G16_WS_BYTES_PER_PROOF / 4), oom)) || (rc = s.slot_to_proof.ensure(slot_cap, oom)) ||
        (rc = s.granule_key.ensure(slot_cap / G16_KEYS_GRANULE + 1, oom)) || (rc = s.slot_status.ensure(slot_cap + 256, oom)))
      return rc;
    s.slot_cap = slot_cap; s.cap_n = n;
  }
  if ((flags & BN254_FLAG_COMPRESSED_PROOFS) && n > s.cmp_cap) {
    s.cmp_cap = 0;
    if ((rc = s.cmp.ensure(bn254::g16_round256(n) * 257, oom))) return rc;
    s.cmp_cap = n;
  }
  return BN254_OK;
}

// Enqueue one batch on `user`.  Caller holds s.mu and has called ensure_set with the batch's flags.  exact_slots: the batch's slots where the caller knows them (the
// host-buffer entry has counted the index), 0: only the device will know -- the launches then cover keys_slot_bound(n, n_keys) slots and the wavefronts past the real
// figure leave at once.  Chunks of G16_MAX_BATCH SLOTS share the workspace; a chunk's sub-batches run side by side on `user` and the set's second stream, as in
// g16_enqueue_exact; both cuts are multiples of 256 slots, so they fall inside a key's run but never inside a granule.
int keys_enqueue(KeySet& s, const void* d_key_index, const void* d_proofs, size_t proof_stride, const void* d_inputs, size_t input_stride, size_t n, void* d_status, hipStream_t user,
                 unsigned flags, size_t exact_slots) {
  const int n_streams = sub_batch_streams() < 2 ? sub_batch_streams() : 2;
  const uint32_t n_keys = (uint32_t)s.list.size();
  const size_t bound = (size_t)bn254::keys_slot_bound(n, n_keys);
  if (n > s.cap_n || bound > s.slot_cap) return set_err(BN254_E_BAD_ARG, "buffers of the key set smaller than the batch (internal sizing error)");
  if (s.busy_valid) HIPCK(hipStreamWaitEvent(user, s.busy_ev, 0));
  const int form = keys_form(n);
  const uint8_t* proofs = (const uint8_t*)d_proofs;
  uint8_t* pre = nullptr;
  if (flags & BN254_FLAG_COMPRESSED_PROOFS) {
    // the decompression never sees a key: the whole batch in proof order first (slots of a chunk refer to proofs anywhere in it), MALFORMED merged at the end
    if (n > s.cmp_cap) return set_err(BN254_E_BAD_ARG, "decompression scratch smaller than the batch (internal sizing error)");
    pre = s.cmp + bn254::g16_round256(s.cmp_cap) * 256;
    for (size_t off = 0; off < n; off += G16_MAX_BATCH) {
      const size_t m = n - off < (size_t)G16_MAX_BATCH ? n - off : (size_t)G16_MAX_BATCH;
      hipError_t e = bn254_launch_g16_decompress(proofs + off * proof_stride, proof_stride, (uint32_t)m, s.cmp + off * 256, pre + off, user);
      if (e != hipSuccess) return launch_err(e, "decompress");
    }
    proofs = s.cmp; proof_stride = 256;
  }
  hipError_t e = hipSuccess;
  if (form == bn254::G16_KEYS_FORM_DIRECT) {
    // one launch group over the n proofs on the caller's stream, at the start of the workspace: a slot is a proof, the status bytes are the caller's
    if (bn254::g16_round256(n) > s.ws_slots()) return set_err(BN254_E_BAD_ARG, "workspace of the key set smaller than the batch (internal sizing error)");
    G16KeysDirectArgs a;
    a.proofs = proofs; a.stride = proof_stride; a.inputs = (const uint8_t*)d_inputs; a.input_stride = input_stride; a.n = n; a.key_index = (const uint32_t*)d_key_index;
    a.desc = s.desc; a.n_keys = n_keys; a.ws = s.ws; a.status = (uint8_t*)d_status; a.strict_scalars = (flags & BN254_FLAG_STRICT_SCALARS) ? 1 : 0;
    if ((e = bn254_launch_g16_keys_direct(a, user)) != hipSuccess) return launch_err(e, "key-set pipeline (direct form)");
  } else {
    e = bn254_launch_keys_group((const uint32_t*)d_key_index, (uint32_t)n, n_keys, (uint32_t)bound, s.count, s.base, s.cursor, s.n_slots, s.slot_to_proof, s.granule_key,
                                (uint8_t*)d_status, user);
    if (e != hipSuccess) return launch_err(e, "grouping");
    const size_t slots = exact_slots ? exact_slots : bound;
    for (size_t off = 0; off < slots; off += G16_MAX_BATCH) {
      const size_t m = slots - off < (size_t)G16_MAX_BATCH ? slots - off : (size_t)G16_MAX_BATCH;
      bn254::G16ChunkPlan plan;
      if (!bn254::g16_plan_chunk(plan, m, 0, 0, n_streams, false)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
      if (bn254::g16_round256(m) > s.ws_slots()) return set_err(BN254_E_BAD_ARG, "workspace of the key set smaller than the batch (internal sizing error)");
      if (plan.concurrent) HIPCK(hipEventRecord(s.fork_ev, user));
      for (int pi = 0; pi < plan.parts; pi++) {
        const size_t lo = plan.part[pi].first, cnt = plan.part[pi].count;
        hipStream_t st = (plan.concurrent && (pi & 1)) ? (hipStream_t)s.aux : user;
        if (st != user && pi == 1) HIPCK(hipStreamWaitEvent(st, s.fork_ev, 0));
        G16KeysLaunchArgs a;
        a.proofs = proofs; a.stride = proof_stride; a.inputs = (const uint8_t*)d_inputs; a.input_stride = input_stride; a.n_proofs = (uint32_t)n;
        a.m = cnt; a.slot0 = (uint32_t)(off + lo); a.n_slots = s.n_slots; a.slot_to_proof = s.slot_to_proof + off + lo; a.granule_key = s.granule_key + (off + lo) / G16_KEYS_GRANULE;
        a.desc = s.desc; a.n_keys = n_keys; a.ws = s.ws + lo * (size_t)(G16_WS_BYTES_PER_PROOF / 4); a.slot_status = s.slot_status + off + lo; a.status = (uint8_t*)d_status;
        a.strict_scalars = (flags & BN254_FLAG_STRICT_SCALARS) ? 1 : 0;
        a.part_of_larger = plan.parts > 1 ? 1 : 0;
        if ((e = bn254_launch_g16_keys(a, st)) != hipSuccess) return launch_err(e, "key-set pipeline");
      }
      if (plan.concurrent && plan.parts > 1) { HIPCK(hipEventRecord(s.join_ev, s.aux)); HIPCK(hipStreamWaitEvent(user, s.join_ev, 0)); }
    }
  }
  if (pre)
    for (size_t off = 0; off < n; off += G16_MAX_BATCH) {
      const size_t m = n - off < (size_t)G16_MAX_BATCH ? n - off : (size_t)G16_MAX_BATCH;
      if ((e = bn254_launch_g16_status_merge((uint8_t*)d_status + off, pre + off, (uint32_t)m, user)) != hipSuccess) return launch_err(e, "status merge");
    }
  HIPCK(hipEventRecord(s.busy_ev, user));
  s.busy_valid = true;
  s.last_form = form;
  return BN254_OK;
}

}  // namespace

// The loader of the grouped form alone, for bn254_dbg_g16_loader_keys (bn254_capi_dbg.hip): the front of keys_enqueue's grouped branch -- bn254_launch_keys_group, then
// bn254_launch_g16_prepare_keys over the batch's slots as ONE launch part -- on the null stream, and the slots read back.  slots: the exact count (a multiple of 64)
int g16_keys_probe_loader(const bn254_g16_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                          size_t input_stride, size_t n, unsigned flags, int misalign, size_t slots, unsigned* out_slot_proof, uint8_t* out_slot_status, uint8_t* out_points,
                          size_t* out_n_slots, int device, void (*points)(const uint8_t*, size_t, uint8_t*)) {
  size_t max_public = 0;
  int rc = check_key_list(pvks, n_keys, &max_public);
  if (rc || (rc = check_device(device))) return rc;
  std::shared_ptr<KeySet> sp = set_cache().get(pvks, n_keys, device, max_public);
  KeySet& s = *sp;
  std::lock_guard<std::mutex> lk(s.mu);
  if ((rc = ensure_set(s, n, flags))) return rc;
  const size_t bound = (size_t)bn254::keys_slot_bound(n, n_keys);
  if (slots == 0 || slots > bound || bound > s.slot_cap || bn254::g16_round256(slots) > s.ws_slots()) return set_err(BN254_E_BAD_ARG, "buffers of the key set smaller than the batch (internal sizing error)");
  const size_t in_bytes = max_public ? (n - 1) * input_stride + 32 * max_public : 0, pb = (n - 1) * proof_stride + 256;
  DevBuf<uint8_t> d_proofs, d_inputs, d_status, d_out; DevBuf<uint32_t> d_index;
  const int oom = BN254_E_NOMEM;
  if ((rc = d_proofs.ensure(pb, oom)) || (rc = d_inputs.ensure(in_bytes + 8, oom)) || (rc = d_index.ensure(n, oom)) || (rc = d_status.ensure(n, oom)) || (rc = d_out.ensure(384 * slots, oom)))
    return rc;
  HIPCK(hipDeviceSynchronize());                                       // the set's buffers may still serve an earlier batch on another stream
  HIPCK(hipMemsetAsync(s.ws, 0, bn254::g16_round256(slots) * (size_t)G16_WS_BYTES_PER_PROOF, nullptr));
  HIPCK(hipMemcpy(d_proofs, proofs, pb, hipMemcpyHostToDevice));
  if (in_bytes) HIPCK(hipMemcpy(d_inputs + misalign, public_inputs, in_bytes, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(d_index, key_index, n * 4, hipMemcpyHostToDevice));
  hipError_t e = bn254_launch_keys_group(d_index, (uint32_t)n, (uint32_t)n_keys, (uint32_t)bound, s.count, s.base, s.cursor, s.n_slots, s.slot_to_proof, s.granule_key, d_status, nullptr);
  if (e != hipSuccess) return launch_err(e, "grouping");
  G16KeysLaunchArgs a;
  a.proofs = d_proofs; a.stride = proof_stride; a.inputs = d_inputs + misalign; a.input_stride = input_stride; a.n_proofs = (uint32_t)n;
  a.m = slots; a.slot0 = 0; a.n_slots = s.n_slots; a.slot_to_proof = s.slot_to_proof; a.granule_key = s.granule_key;
  a.desc = s.desc; a.n_keys = (uint32_t)n_keys; a.ws = s.ws; a.slot_status = s.slot_status; a.status = d_status;
  a.strict_scalars = (flags & BN254_FLAG_STRICT_SCALARS) ? 1 : 0;
  bn254_launch_g16_prepare_keys(a, (unsigned)((slots + 255) / 256), nullptr);
  if ((e = hipGetLastError()) == hipSuccess) e = bn254_launch_dbg_store(s.ws, slots, (int)bn254::VE_AX, d_out, 0, nullptr);
  if (e != hipSuccess) return launch_err(e, "key-set loader");
  HIPCK(hipDeviceSynchronize());
  std::vector<uint8_t> stored(384 * slots);
  uint32_t ns = 0;
  HIPCK(hipMemcpy(stored.data(), d_out, 384 * slots, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(out_slot_proof, s.slot_to_proof, slots * 4, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(out_slot_status, s.slot_status, slots, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(&ns, s.n_slots, 4, hipMemcpyDeviceToHost));
  points(stored.data(), slots, out_points);
  *out_n_slots = ns;
  return BN254_OK;
}

// bn254_groth16_vk_free: every cached set that contains the key goes
void keys_sets_drop(const bn254_g16_pvk* member) { set_cache().drop(member); }

extern "C" {

int bn254_groth16_reserve_keys(const bn254_g16_pvk* const* pvks, size_t n_keys, size_t n, int device) {
  size_t max_public = 0;
  int rc = check_key_list(pvks, n_keys, &max_public);
  if (rc) return rc;
  if ((rc = check_device(device))) return rc;
  std::shared_ptr<KeySet> s = set_cache().get(pvks, n_keys, device, max_public);
  std::lock_guard<std::mutex> lk(s->mu);
  return ensure_set(*s, n ? n : 1, 0);
}

int bn254_groth16_verify_batch_keys_device(const bn254_g16_pvk* const* pvks, size_t n_keys, const void* d_key_index, const void* d_proofs, size_t proof_stride,
                                           const void* d_public_inputs, size_t input_stride, size_t n, void* d_status, int device, void* hip_stream, unsigned flags) {
  size_t max_public = 0;
  int rc = check_keys_args(pvks, n_keys, d_key_index, d_proofs, proof_stride, d_public_inputs, input_stride, n, d_status, flags, &max_public);
  if (rc || n == 0) return rc;
  if ((rc = check_device(device))) return rc;
  std::shared_ptr<KeySet> s = set_cache().get(pvks, n_keys, device, max_public);
  std::lock_guard<std::mutex> lk(s->mu);
  if ((rc = ensure_set(*s, n, flags))) return rc;
  return keys_enqueue(*s, d_key_index, d_proofs, proof_stride, d_public_inputs, input_stride, n, d_status, (hipStream_t)hip_stream, flags, 0);
}

// Host buffers.  Grouping is global (a chunk of slots refers to proofs anywhere in the batch), so this entry uploads everything first -- index, records and input rows
// through a ring of pinned pieces on a copy stream, the host threads filling piece i + 1 while piece i travels -- and then runs the device entry's pipeline on the
// copies.  The index is counted on the host beforehand: that is the range check the device entry cannot make, and it gives the exact number of slots, so no launch
// covers slots that do not exist.
int bn254_groth16_verify_batch_keys(const bn254_g16_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride,
                                    const uint8_t* public_inputs, size_t input_stride, size_t n, uint8_t* status, int device, unsigned flags) {
  size_t max_public = 0;
  int rc = check_keys_args(pvks, n_keys, key_index, proofs, proof_stride, public_inputs, input_stride, n, status, flags, &max_public);
  if (rc || n == 0) return rc;
  size_t exact_slots = 0;
  {
    std::vector<uint32_t> count(n_keys, 0);
    for (size_t i = 0; i < n; i++) {
      if (key_index[i] >= n_keys) return set_err(BN254_E_BAD_ARG, "key_index[" + std::to_string(i) + "] = " + std::to_string(key_index[i]) + " is outside the list of " + std::to_string(n_keys) + " keys");
      count[key_index[i]]++;
    }
    for (size_t k = 0; k < n_keys; k++) exact_slots += bn254::keys_round_up(count[k]);
  }
  if ((rc = check_device(device))) return rc;
  std::shared_ptr<KeySet> sp = set_cache().get(pvks, n_keys, device, max_public);
  KeySet& s = *sp;
  std::lock_guard<std::mutex> lk(s.mu);
  if ((rc = ensure_set(s, n, flags))) return rc;
  const size_t in_bytes = max_public ? n * input_stride : 0;
  const int oom = BN254_E_NOMEM;
  if ((rc = s.st_proofs.ensure(n * proof_stride, oom)) || (rc = s.st_inputs.ensure(in_bytes ? in_bytes : 32, oom)) || (rc = s.st_index.ensure(n * 4, oom)) ||
      (rc = s.st_status.ensure(n, oom)) || (rc = s.ring.ensure(KEYS_HOST_PIECE)))
    return rc;
  PinRing& ring = s.ring;
  ring.begin();
  auto push = [&](uint8_t* dst, const uint8_t* src, size_t len) { return ring.push(dst, len, [src](uint8_t* q, size_t from, size_t k) { parallel_copy(q, src + from, k); }); };
  // the staging buffers may still be read by the previous batch of this set: the copies start after it
  if (s.busy_valid) HIPCK(hipStreamWaitEvent(ring.copy, s.busy_ev, 0));
  if ((rc = push(s.st_index, (const uint8_t*)key_index, n * 4)) || (rc = push(s.st_proofs, proofs, n * proof_stride)) || (in_bytes && (rc = push(s.st_inputs, public_inputs, in_bytes))))
    return ring.drain(rc);
  if (ring.last()) HIPCK(hipStreamWaitEvent(ring.compute, ring.last(), 0));
  if ((rc = keys_enqueue(s, s.st_index, s.st_proofs, proof_stride, s.st_inputs, input_stride, n, s.st_status, ring.compute, flags, exact_slots))) return ring.drain(rc);
  HIPCK(hipMemcpyAsync(status, s.st_status, n, hipMemcpyDeviceToHost, ring.compute));
  HIPCK(hipStreamSynchronize(ring.compute));
  return BN254_OK;
}

void bn254_set_keys_params(long coop_max) {
  if (coop_max >= 0) g_keys_coop_max.store(keys_coop_clamp(coop_max), std::memory_order_relaxed);
}

// The plan of a batch, for the tests: the form from the function keys_enqueue calls, and what that form enqueues for raw records through the device entry (which
// covers keys_slot_bound(n, n_keys) slots).  The grouped form's kernels are counted by walking its programs with an operation counter.
namespace {
struct KeysCountOps {
  int launches = 0;
  void miller_run(int, int, int, int, int, int, int, int) { launches++; }
  void f12_mul(int, int, int, bool = false) { launches++; }
  void f12_cyclo_sqr(int, int) { launches++; }
  void f12_cyclo_sqr_n(int, int, int) { launches++; }
  void f12_frob(int, int, int) { launches++; }
  void f12_inv(int, int) { launches++; }
};
}  // namespace
int bn254_dbg_g16_keys_plan(size_t n, size_t n_keys, int* form, size_t* slots, int* launches) {
  if (!form || !slots || !launches || n == 0 || n_keys == 0 || n_keys > G16_KEYS_MAX_KEYS || bn254::keys_slot_bound(n, n_keys) > 0xffff0000ull) return set_err(BN254_E_BAD_ARG, "bad argument");
  *form = keys_form(n);
  if (*form == bn254::G16_KEYS_FORM_DIRECT) { *slots = n; *launches = 2; return BN254_OK; }      // k_g16_prepare, k_coop12_miller_g16_keys
  const size_t bound = (size_t)bn254::keys_slot_bound(n, n_keys);
  const int n_streams = sub_batch_streams() < 2 ? sub_batch_streams() : 2;
  int total = 6;                                   // bn254_launch_keys_group: three memsets, count, scan, place
  for (size_t off = 0; off < bound; off += G16_MAX_BATCH) {
    const size_t m = bound - off < (size_t)G16_MAX_BATCH ? bound - off : (size_t)G16_MAX_BATCH;
    bn254::G16ChunkPlan plan;
    if (!bn254::g16_plan_chunk(plan, m, 0, 0, n_streams, false)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
    for (int pi = 0; pi < plan.parts; pi++) {
      KeysCountOps ops;
      bn254::vm_miller_program_runs(ops, bn254::g16_launch_form(plan.part[pi].count, 0, true, false, plan.parts > 1, false, false, -1).run_steps);
      bn254::vm_final_exp_program_head(ops);
      total += 1 + ops.launches + 1;               // k_g16_prepare_keys, the runs and the program, k_f12_mul_verdict_keys
    }
  }
  *slots = bound; *launches = total;
  return BN254_OK;
}
int bn254_dbg_g16_keys_last_form(const bn254_g16_pvk* const* pvks, size_t n_keys, int device, int* form) {
  if (!pvks || !form || n_keys == 0) return set_err(BN254_E_BAD_ARG, "bad argument");
  *form = -1;
  std::shared_ptr<KeySet> s = set_cache().find(pvks, n_keys, device);
  if (s) { std::lock_guard<std::mutex> lk(s->mu); *form = s->last_form; }
  return BN254_OK;
}

// The grouping of a batch, for the tests: device -1 runs the steps on the host (bn254_keys.h::keys_group_host), a device ordinal runs k_keys_count / _scan / _place.
// out_slot_to_proof: bn254_dbg_g16_keys_slot_bound(n, n_keys) words (all ones in padding slots and past out_n_slots), out_granule_key: a word per 64 of them.
size_t bn254_dbg_g16_keys_slot_bound(size_t n, size_t n_keys) { return (size_t)bn254::keys_slot_bound(n, n_keys); }
int bn254_dbg_g16_keys_group(const unsigned* key_index, size_t n, size_t n_keys, int device, unsigned* out_slot_to_proof, unsigned* out_granule_key, size_t* out_n_slots) {
  if (!key_index || !out_slot_to_proof || !out_granule_key || !out_n_slots || n == 0 || n_keys == 0 || n_keys > G16_KEYS_MAX_KEYS || bn254::keys_slot_bound(n, n_keys) > 0xffff0000ull)
    return set_err(BN254_E_BAD_ARG, "bad argument");
  const size_t bound = (size_t)bn254::keys_slot_bound(n, n_keys), granules = bound / G16_KEYS_GRANULE;
  if (device < 0) {
    std::vector<uint32_t> count(n_keys), base(n_keys);
    for (size_t sidx = 0; sidx < bound; sidx++) out_slot_to_proof[sidx] = G16_KEYS_NO_PROOF;
    for (size_t g = 0; g < granules; g++) out_granule_key[g] = 0;
    *out_n_slots = bn254::keys_group_host(key_index, (uint32_t)n, (uint32_t)n_keys, out_slot_to_proof, out_granule_key, count.data(), base.data());
    return BN254_OK;
  }
  int rc = check_device(device);
  if (rc) return rc;
  DevBuf<uint32_t> idx, cnt, s2p, gk; DevBuf<uint8_t> st;
  const int oom = BN254_E_NOMEM;
  if ((rc = idx.ensure(n, oom)) || (rc = cnt.ensure(3 * n_keys + 1, oom)) || (rc = s2p.ensure(bound, oom)) || (rc = gk.ensure(granules + 1, oom)) || (rc = st.ensure(n, oom))) return rc;
  hipError_t e = hipMemcpy(idx, key_index, n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = bn254_launch_keys_group(idx, (uint32_t)n, (uint32_t)n_keys, (uint32_t)bound, cnt, cnt + n_keys, cnt + 2 * n_keys, cnt + 3 * n_keys, s2p, gk, st, nullptr);
  uint32_t ns = 0;
  if (e == hipSuccess) e = hipMemcpy(&ns, cnt + 3 * n_keys, 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_slot_to_proof, s2p, bound * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_granule_key, gk, granules * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("grouping: ") + hipGetErrorString(e));
  *out_n_slots = ns;
  return BN254_OK;
}

}  // extern "C"
