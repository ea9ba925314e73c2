// bn254_capi_pairing.hip -- the batch pairing product over caller-supplied (G1, G2) pairs (include/bn254_verify.h: bn254_pairing_check_batch, _device,
// bn254_pairing_batch, bn254_pairing_reserve; the knob and the counters of a launch's form: bn254_set_pairing_params, bn254_pairing_params, bn254_pairing_state) and its
// probes bn254_dbg_pairing_batch, bn254_dbg_pairing_batch_form, bn254_dbg_pairing_form, bn254_dbg_pairing_plan.  No key: one workspace per DEVICE, shared by every call on it, so calls on a
// device are serialised the way a (key, device) is in the Groth16 entries -- the enqueue under the device's lock, after a wait (on the GPU) for the completion event
// of the previous call.
// The same entries for items whose G2 point of some positions is shared by the whole batch and prepared (bn254_g2_prepare, bn254_pairing_check_batch_shared, _device,
// bn254_pairing_batch_shared, the probe bn254_dbg_pairing_batch_shared): PbShared carries the mask and the records through the same checks, passes and launches.
// Not part of the one-translation-unit host build of bn254_capi.hip (tests/hostsan/hostsan_main.cpp): a harness that wants it includes this file itself
// (tests/hostsan/hostsan_pairing.cpp, hostsan_pairing_shared.cpp).
#include "bn254_capi_internal.h"
#include "bn254_pairing_batch.h"
#include "bn254_capi_pairing.h"

// items per pass: what the workspace of a device holds at most (1.2 GB) and what one launch works on
#define PB_PASS_ITEMS ((size_t)1 << 18)
// the host entries stage a pass's records through pinned memory of at most this many bytes: 2^18 items of one pair, 32 768 items of eight
#define PB_STAGE_BYTES ((size_t)48 << 20)

// BN254_PAIRING_PASS (tests; read once when the library is loaded) lowers the items per pass, 64 at least
static const size_t g_pb_pass_items = [] { long v = env_long("BN254_PAIRING_PASS", (long)PB_PASS_ITEMS); return (size_t)(v < 64 ? 64 : (v > (long)PB_PASS_ITEMS ? (long)PB_PASS_ITEMS : v)); }();

// The knob of a launch's form (bn254_set_pairing_params; BN254_PAIRING_COOP_MAX gives the initial value once, at load time): launches of up to this many items take the
// cooperative form (k_coop12_miller_pairs), larger ones the lane form; 0: always the lane form.  BN254_COOP=0 switches it off (bn254_g16_plan.h::pairing_form)
static long pb_coop_clamp(long v) { return v > (long)COOP12_MAX_PROOFS ? (long)COOP12_MAX_PROOFS : v; }
static std::atomic<long> g_pb_coop_max{[] { long v = env_long("BN254_PAIRING_COOP_MAX", (long)PAIRING_COOP_MAX_DEFAULT); return v < 0 ? (long)PAIRING_COOP_MAX_DEFAULT : pb_coop_clamp(v); }()};
int pb_form(size_t n_pairs, size_t n) { return bn254::pairing_form(n_pairs, n, (size_t)g_pb_coop_max.load(std::memory_order_relaxed), bn254::knob_coop_on()); }
// bn254_pairing_state: launches enqueued so far in the cooperative | the lane form
static std::atomic<uint64_t> g_pb_launches[2];
void pb_count_launch(int form) { g_pb_launches[form == bn254::PAIRING_FORM_COOP ? 0 : 1].fetch_add(1, std::memory_order_relaxed); }

// The passes of a call, without a device (bn254_dbg_pairing_plan reads the same functions).  ws_items: the workspace a reservation of n items allocates; host_pass:
// the items per pass of the host entries, every one of which fits that reservation
static inline size_t pb_ws_items(size_t n) { return n < g_pb_pass_items ? n : g_pb_pass_items; }
size_t pb_ws_items_of(size_t n) { return pb_ws_items(n); }
// rec: the bytes of an item as staged; lead: bytes staged in front of a pass's items (the prepared records of a call with shared positions)
size_t pb_host_pass_of(size_t rec, size_t lead, size_t n) {
  size_t pass = (PB_STAGE_BYTES - lead) / rec;
  if (pass > g_pb_pass_items) pass = g_pb_pass_items;
  return n < pass ? n : pass;
}
static inline size_t pb_host_pass(size_t n_pairs, size_t n) { return pb_host_pass_of((size_t)PB_PAIR_LEN * n_pairs, 0, n); }

// never destroyed (device memory must not be freed from a static destructor: bn254_capi_internal.h, KeyCache); map nodes never move
PbDev* pb_dev(int device) {
  static std::mutex mu;
  static std::map<int, PbDev>* devs = new std::map<int, PbDev>();
  std::lock_guard<std::mutex> lk(mu);
  return &(*devs)[device];
}
// caller holds d.mu: the device made ready (self-test at its first use) and the workspace grown to what a reservation of n items holds
int pb_ensure(PbDev& d, int device, size_t n) {
  int rc = check_device(device);
  if (rc || (rc = selftest_gate(device))) return rc;
  if (!d.ready) {
    std::vector<int32_t> one(12 * BN_NL);
    put_fp12(one.data(), bn254::fp12_one());
    if ((rc = upload(d.one, one)) || (rc = d.busy_ev.ensure())) return rc;
    d.ready = true;
  }
  return d.ws.ensure(pb_ws_items(n) * (size_t)(G16_WS_BYTES_PER_PROOF / 4));
}
namespace {

// caller holds d.mu; everything on `user`, nothing allocated.  verdict: the status bytes are ACCEPT / REJECT; d_gt (may be null): the GT values
// force: PAIRING_FORM_PLAN, or the form every launch takes (the probe; the caller has checked n against the cooperative range).  A launch is never split between forms
int pb_enqueue(PbDev& d, const uint8_t* d_pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* d_status, uint8_t* d_gt, bool verdict, hipStream_t user,
               int force = bn254::PAIRING_FORM_PLAN, const PbShared& sh = PbShared()) {
  const size_t cap = d.ws_items();
  if (cap == 0) return set_err(BN254_E_BAD_ARG, "pairing workspace not allocated (internal sizing error)");
  if (d.busy_valid) HIPCK(hipStreamWaitEvent(user, d.busy_ev, 0));
  for (size_t off = 0; off < n; off += cap) {
    bn254::PairingLaunchArgs a;
    a.pairs = d_pairs + off * item_stride; a.item_stride = item_stride; a.n_pairs = (int)n_pairs; a.n = n - off < cap ? n - off : cap;
    a.ws = d.ws; a.status = d_status + off; a.one = verdict ? (const int32_t*)d.one : nullptr; a.out_gt = d_gt ? d_gt + 384 * off : nullptr;
    a.form = force != bn254::PAIRING_FORM_PLAN ? force : pb_form(n_pairs, a.n);
    a.shared_mask = sh.mask; a.prepared = (const int32_t*)sh.prepared;
    const hipError_t e = bn254_launch_pairing_batch(a, user);
    if (e != hipSuccess) return launch_err(e, "pairing batch");
    pb_count_launch(a.form);
  }
  HIPCK(hipEventRecord(d.busy_ev, user));
  d.busy_valid = true;
  return BN254_OK;
}

}  // namespace

// BN254_E_BAD_ARG before any device is touched; *done: n == 0, nothing to do
// sh: the shared positions (the _shared entries); host_records: sh.prepared is host memory, so the header words of its records are checked here as well
int pb_check_args(const void* pairs, size_t item_stride, size_t n_pairs, size_t n, const void* status, const void* out_gt, bool wants_gt, bool* done,
                  const PbShared& sh, bool host_records) {
  *done = false;
  if (n_pairs < 1 || n_pairs > BN254_PAIRING_MAX_PAIRS) return set_err(BN254_E_BAD_ARG, "bad argument: n_pairs is 1 .. 8");
  if (sh.mask >> n_pairs) return set_err(BN254_E_BAD_ARG, "bad argument: shared_mask has a bit at or above n_pairs");
  if (sh.mask) {
    if (!sh.prepared) return set_err(BN254_E_BAD_ARG, "bad argument: shared_mask without prepared records");
    if (item_stride < bn254::pb_item_len((int)n_pairs, sh.mask)) return set_err(BN254_E_BAD_ARG, "bad argument: item_stride below the packed item (64 bytes per shared position, 192 per variable one)");
    if (!host_records && ((uintptr_t)sh.prepared & 3)) return set_err(BN254_E_BAD_ARG, "bad argument: d_prepared is not 4-byte aligned");
    if (host_records)
      for (size_t t = 0; t < sh.count(); t++) {
        uint32_t h[2];
        memcpy(h, sh.prepared + t * PB_PREP_LEN, sizeof h);
        if (h[0] != PB_PREP_MAGIC || h[1] != PB_PREP_VERSION) return set_err(BN254_E_BAD_ARG, "bad argument: a prepared G2 record with a wrong magic word or layout version (bn254_g2_prepare of this library writes it)");
      }
  } else if (item_stride < (size_t)BN254_PAIRING_PAIR_LEN * n_pairs) return set_err(BN254_E_BAD_ARG, "bad argument: item_stride below 192 * n_pairs");
  if (n && (!pairs || !status || (wants_gt && !out_gt))) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n && item_stride > SIZE_MAX / n) return set_err(BN254_E_BAD_ARG, "bad argument: n items of item_stride bytes overflow the address space");
  *done = n == 0;
  return BN254_OK;
}

namespace {

// a host-buffer call: passes of pb_host_pass items through the pinned staging; returns with the status bytes (and GT values) of every item
// sh: the prepared records (host memory) travel in front of every pass's items, in the same pinned buffer and the same copy; the items are then the packed ones
int pb_host_call(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* out_gt, uint8_t* status, int device, bool verdict, int force = bn254::PAIRING_FORM_PLAN,
                 const PbShared& sh = PbShared()) {
  PbDev* d = pb_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  const size_t rec = bn254::pb_item_len((int)n_pairs, sh.mask), lead = sh.bytes(), pass = pb_host_pass_of(rec, lead, n);
  static_assert(PB_PREP_LEN % 16 == 0, "the items behind the prepared records keep the staging buffer's alignment");
  int rc;
  if ((rc = pb_ensure(*d, device, pass)) || (rc = d->stream.ensure())) return rc;
  if ((rc = d->h_in.ensure(lead + pass * rec)) || (rc = d->h_status.ensure(pass)) || (rc = d->d_in.ensure(lead + pass * rec)) || (rc = d->d_status.ensure(pass))) return rc;
  if (out_gt && ((rc = d->h_gt.ensure(pass * 384)) || (rc = d->d_gt.ensure(pass * 384)))) return rc;
  hipStream_t s = d->stream;
  auto one_pass = [&](size_t off, size_t m) -> int {
    if (lead) memcpy(d->h_in, sh.prepared, lead);
    if (item_stride == rec) parallel_copy(d->h_in + lead, pairs + off * rec, m * rec);
    else for (size_t i = 0; i < m; i++) memcpy(d->h_in + lead + i * rec, pairs + (off + i) * item_stride, rec);
    HIPCK(hipMemcpyAsync(d->d_in, d->h_in, lead + m * rec, hipMemcpyHostToDevice, s));
    int r = pb_enqueue(*d, d->d_in + lead, rec, n_pairs, m, d->d_status, out_gt ? (uint8_t*)d->d_gt : nullptr, verdict, s, force, PbShared{sh.mask, sh.mask ? (const uint8_t*)d->d_in : nullptr});
    if (r) return r;
    HIPCK(hipMemcpyAsync(d->h_status, d->d_status, m, hipMemcpyDeviceToHost, s));
    if (out_gt) HIPCK(hipMemcpyAsync(d->h_gt, d->d_gt, m * 384, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    memcpy(status + off, d->h_status, m);
    if (out_gt) memcpy(out_gt + 384 * off, d->h_gt, m * 384);
    return BN254_OK;
  };
  for (size_t off = 0; off < n; off += pass) {
    if ((rc = one_pass(off, n - off < pass ? n - off : pass))) {
      const std::string keep = g_err;      // the staging must be quiescent when the lock is released; the failure's text is the one the caller reads
      (void)hipStreamSynchronize(s);
      return set_err(rc, keep);
    }
  }
  return BN254_OK;
}

}  // namespace

extern "C" {

int bn254_pairing_reserve(size_t n, int device) {
  PbDev* d = pb_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  return pb_ensure(*d, device, n ? n : 1);
}

int bn254_pairing_check_batch(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* status, int device) {
  bool done;
  int rc = pb_check_args(pairs, item_stride, n_pairs, n, status, nullptr, false, &done);
  if (rc || done) return rc;
  return pb_host_call(pairs, item_stride, n_pairs, n, nullptr, status, device, true);
}

int bn254_pairing_check_batch_device(const void* d_pairs, size_t item_stride, size_t n_pairs, size_t n, void* d_status, int device, void* hip_stream) {
  bool done;
  int rc = pb_check_args(d_pairs, item_stride, n_pairs, n, d_status, nullptr, false, &done);
  if (rc || done) return rc;
  PbDev* d = pb_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  // no allocation when the workspace already holds min(n, PB_PASS_ITEMS) items (bn254_pairing_reserve, or an earlier call of that size); a batch above
  // PB_PASS_ITEMS runs as several launches, one after the other
  if ((rc = pb_ensure(*d, device, n))) return rc;
  return pb_enqueue(*d, (const uint8_t*)d_pairs, item_stride, n_pairs, n, (uint8_t*)d_status, nullptr, true, (hipStream_t)hip_stream);
}

int bn254_pairing_batch(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* out_gt, uint8_t* status, int device) {
  bool done;
  int rc = pb_check_args(pairs, item_stride, n_pairs, n, status, out_gt, true, &done);
  if (rc || done) return rc;
  return pb_host_call(pairs, item_stride, n_pairs, n, out_gt, status, device, false);
}

// The probe: the status bytes of bn254_pairing_check_batch AND (out_gt non-null) the GT values of bn254_pairing_batch, from one run.  device -1: the host compile of
// the same loader, vm_miller_run_var and final-exponentiation program on plain arrays (bn254_pairing_batch.h::pb_item_on_host), no device touched; a device ordinal:
// the kernels, through the host-buffer path above
int bn254_dbg_pairing_batch(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* out_gt, uint8_t* status, int device) {
  bool done;
  int rc = pb_check_args(pairs, item_stride, n_pairs, n, status, nullptr, false, &done);
  if (rc || done) return rc;
  if (device < -1) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (device >= 0) return pb_host_call(pairs, item_stride, n_pairs, n, out_gt, status, device, true);
  const int run_steps = bn254::knob_run_steps_pairing_batch();      // the loop cut into runs as the launcher cuts it (BN254_MILLER_RUN_STEPS)
  for (size_t i = 0; i < n; i++) status[i] = bn254::pb_item_on_host(pairs + i * item_stride, (int)n_pairs, out_gt ? out_gt + 384 * i : nullptr, run_steps);
  return BN254_OK;
}

// ---- shared, prepared G2 points ---------------------------------------------------------------------------------------------------------------------------------
static_assert(BN254_G2_PREPARED_LEN == PB_PREP_LEN && PB_PREP_LEN == 4 * sizeof(uint32_t) + 4 * sizeof(bn254::Fp::v) + BN_ATE_STEPS * 6 * sizeof(bn254::Fp::v),
              "BN254_G2_PREPARED_LEN is the header of four dwords, the digits of four Fp and of BN_ATE_STEPS lines of three Fp2 (FixedLine: m, c, xc)");
static_assert(sizeof(bn254::FixedLine) == 3 * sizeof(bn254::Fp2) && sizeof(bn254::Fp2) == 2 * sizeof(bn254::Fp), "a line is three Fp2");
static_assert(BN254_PAIRING_G1_LEN == PB_G1_LEN, "a shared position of a packed item");

// Host work, no device: the checks of phase 1 and phase 2 of the definition on one G2 point, then its record -- the Fp values the loader computes from the same
// bytes (so that a workspace filled from the record is the one filled from the bytes) and the 88 affine lines of fixed_line_table in the key tables' encoding
int bn254_g2_prepare(const uint8_t g2[128], uint8_t out[BN254_G2_PREPARED_LEN], uint8_t* status) {
  if (!g2 || !out || !status) return set_err(BN254_E_BAD_ARG, "bad argument");
  bool memb = true, zero = true;
  bn254::G2Aff q;
  q.x.c1 = bn254::pb_field(g2, false, memb, zero); q.x.c0 = bn254::pb_field(g2 + 32, false, memb, zero);
  q.y.c1 = bn254::pb_field(g2 + 64, false, memb, zero); q.y.c0 = bn254::pb_field(g2 + 96, false, memb, zero);
  if (!memb) { *status = BN254_ERR_NOT_MEMBER; return BN254_OK; }
  std::vector<int32_t> rec(PB_PREP_DWORDS, 0);
  rec[0] = (int32_t)PB_PREP_MAGIC; rec[1] = (int32_t)PB_PREP_VERSION; rec[2] = zero ? (int32_t)PB_PREP_FLAG_IDENTITY : 0;
  const bn254::Fp* coord[4] = {&q.x.c0, &q.x.c1, &q.y.c0, &q.y.c1};
  for (int c = 0; c < 4; c++)
    for (int l = 0; l < BN_NL; l++) rec[PB_PREP_HDR_DWORDS + c * BN_NL + l] = coord[c]->v[l];
  if (!zero) {
    if (!bn254::g2_on_curve(q)) { *status = BN254_ERR_NOT_ON_CURVE; return BN254_OK; }
    if (!bn254::g2_in_subgroup(q)) { *status = BN254_ERR_NOT_IN_SUBGROUP; return BN254_OK; }
    std::vector<bn254::FixedLine> tab(BN_ATE_STEPS);
    if (!bn254::fixed_line_table(tab.data(), q)) return set_err(BN254_E_BAD_ARG, "no line table for the G2 point (an exceptional step: unreachable for a point of the r-torsion)");
    for (int s = 0; s < BN_ATE_STEPS; s++) {
      int32_t* e = rec.data() + PB_PREP_HDR_DWORDS + PB_PREP_POINT_DWORDS + (size_t)s * FIXED_LINE_DWORDS;
      put_fp2(e, tab[s].m); put_fp2(e + 2 * BN_NL, tab[s].c); put_fp2(e + 4 * BN_NL, tab[s].xc);
    }
  }
  memcpy(out, rec.data(), PB_PREP_LEN);
  *status = BN254_ACCEPT;
  return BN254_OK;
}

int bn254_pairing_check_batch_shared(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared, size_t n, uint8_t* status, int device) {
  const PbShared sh{shared_mask, shared_mask ? prepared : nullptr};
  bool done;
  int rc = pb_check_args(items, item_stride, n_pairs, n, status, nullptr, false, &done, PbShared{shared_mask, prepared}, true);
  if (rc || done) return rc;
  return pb_host_call(items, item_stride, n_pairs, n, nullptr, status, device, true, bn254::PAIRING_FORM_PLAN, sh);
}

int bn254_pairing_check_batch_shared_device(const void* d_items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const void* d_prepared, size_t n, void* d_status, int device,
                                            void* hip_stream) {
  const PbShared sh{shared_mask, shared_mask ? (const uint8_t*)d_prepared : nullptr};
  bool done;
  int rc = pb_check_args(d_items, item_stride, n_pairs, n, d_status, nullptr, false, &done, PbShared{shared_mask, (const uint8_t*)d_prepared}, false);
  if (rc || done) return rc;
  PbDev* d = pb_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  if ((rc = pb_ensure(*d, device, n))) return rc;
  return pb_enqueue(*d, (const uint8_t*)d_items, item_stride, n_pairs, n, (uint8_t*)d_status, nullptr, true, (hipStream_t)hip_stream, bn254::PAIRING_FORM_PLAN, sh);
}

int bn254_pairing_batch_shared(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared, size_t n, uint8_t* out_gt, uint8_t* status,
                               int device) {
  const PbShared sh{shared_mask, shared_mask ? prepared : nullptr};
  bool done;
  int rc = pb_check_args(items, item_stride, n_pairs, n, status, out_gt, true, &done, PbShared{shared_mask, prepared}, true);
  if (rc || done) return rc;
  return pb_host_call(items, item_stride, n_pairs, n, out_gt, status, device, false, bn254::PAIRING_FORM_PLAN, sh);
}

// The probe of the shared entries, the counterpart of bn254_dbg_pairing_batch[_form]: status bytes of the check AND (out_gt non-null) the GT values from one run.
// device -1 (form 0): the host compile -- pb_load_item_shared, vm_miller_run_mix and the final-exponentiation program on plain arrays, the loop cut by
// BN254_MILLER_RUN_STEPS; a device ordinal: the kernels, form 0 as the plan says, 1 the lane kernels, 2 the cooperative kernel
int bn254_dbg_pairing_batch_shared(const uint8_t* items, size_t item_stride, size_t n_pairs, unsigned shared_mask, const uint8_t* prepared, size_t n, uint8_t* out_gt, uint8_t* status,
                                   int device, int form) {
  const PbShared sh{shared_mask, shared_mask ? prepared : nullptr};
  bool done;
  int rc = pb_check_args(items, item_stride, n_pairs, n, status, nullptr, false, &done, PbShared{shared_mask, prepared}, true);
  if (rc) return rc;
  if (device < -1 || form < 0 || form > bn254::PAIRING_FORM_COOP || (form != bn254::PAIRING_FORM_PLAN && device < 0))
    return set_err(BN254_E_BAD_ARG, "bad argument: form 0 runs anywhere, form 1 (lane) and 2 (cooperative) run on a device");
  if (form == bn254::PAIRING_FORM_COOP && n > (size_t)COOP12_MAX_PROOFS) return set_err(BN254_E_BAD_ARG, "bad argument: the cooperative form takes at most 30 720 items");
  if (done) return BN254_OK;
  if (device >= 0) return pb_host_call(items, item_stride, n_pairs, n, out_gt, status, device, true, form, sh);
  const int run_steps = bn254::knob_run_steps_pairing_batch();
  if (!sh.mask) {
    for (size_t i = 0; i < n; i++) status[i] = bn254::pb_item_on_host(items + i * item_stride, (int)n_pairs, out_gt ? out_gt + 384 * i : nullptr, run_steps);
    return BN254_OK;
  }
  std::vector<int32_t> recs(sh.count() * PB_PREP_DWORDS);      // the caller's bytes need not be aligned
  memcpy(recs.data(), sh.prepared, sh.bytes());
  for (size_t i = 0; i < n; i++) status[i] = bn254::pb_item_shared_on_host(items + i * item_stride, (int)n_pairs, sh.mask, recs.data(), out_gt ? out_gt + 384 * i : nullptr, run_steps);
  return BN254_OK;
}

// bn254_dbg_pairing_batch with the form of every launch forced: 0 as that probe (device -1: the host compile), 1 the lane kernels, 2 the cooperative kernel
int bn254_dbg_pairing_batch_form(const uint8_t* pairs, size_t item_stride, size_t n_pairs, size_t n, uint8_t* out_gt, uint8_t* status, int device, int form) {
  if (form == bn254::PAIRING_FORM_PLAN) return bn254_dbg_pairing_batch(pairs, item_stride, n_pairs, n, out_gt, status, device);
  bool done;
  int rc = pb_check_args(pairs, item_stride, n_pairs, n, status, nullptr, false, &done);
  if (rc) return rc;
  if ((form != bn254::PAIRING_FORM_LANES && form != bn254::PAIRING_FORM_COOP) || device < 0) return set_err(BN254_E_BAD_ARG, "bad argument: form 1 (lane) and 2 (cooperative) run on a device");
  if (form == bn254::PAIRING_FORM_COOP && n > (size_t)COOP12_MAX_PROOFS) return set_err(BN254_E_BAD_ARG, "bad argument: the cooperative form takes at most 30 720 items");
  if (done) return BN254_OK;
  return pb_host_call(pairs, item_stride, n_pairs, n, out_gt, status, device, true, form);
}
// the plan's answer for a launch of n items of n_pairs pairs under the knobs as they are now (1 lane, 2 cooperative); no device touched
int bn254_dbg_pairing_form(size_t n_pairs, size_t n, int* form) {
  if (!form || n_pairs < 1 || n_pairs > BN254_PAIRING_MAX_PAIRS) return set_err(BN254_E_BAD_ARG, "bad argument");
  *form = pb_form(n_pairs, n);
  return BN254_OK;
}

void bn254_set_pairing_params(long coop_max) {
  if (coop_max >= 0) g_pb_coop_max.store(pb_coop_clamp(coop_max));
}
int bn254_pairing_params(long out[1]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  out[0] = g_pb_coop_max.load();
  return BN254_OK;
}
int bn254_pairing_state(uint64_t out[2]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  for (int i = 0; i < 2; i++) out[i] = g_pb_launches[i].load(std::memory_order_relaxed);
  return BN254_OK;
}

// host-only probe of the pass plan: for a call of n items of n_pairs pairs -- out = {items a reservation of n allocates workspace for, items per pass of the host
// entries, passes of the host entries, pinned bytes of a pass's records}
int bn254_dbg_pairing_plan(size_t n_pairs, size_t n, uint64_t out[4]) {
  if (!out || n_pairs < 1 || n_pairs > BN254_PAIRING_MAX_PAIRS) return set_err(BN254_E_BAD_ARG, "bad argument");
  const size_t pass = pb_host_pass(n_pairs, n);
  out[0] = pb_ws_items(n); out[1] = pass; out[2] = pass ? (n + pass - 1) / pass : 0; out[3] = (uint64_t)pass * PB_PAIR_LEN * n_pairs;
  return BN254_OK;
}

}  // extern "C"
