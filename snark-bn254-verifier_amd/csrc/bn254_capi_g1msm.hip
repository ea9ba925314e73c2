// bn254_capi_g1msm.hip -- batch G1 multi-scalar multiplication with per-item and shared bases (include/bn254_verify.h: bn254_g1_bases_prepare, _free, _count,
// bn254_g1_msm_batch, _device, bn254_g1_msm_reserve) and its probe bn254_dbg_g1_msm_batch.  A per-DEVICE workspace of its own (term records, rows, window-table scratch,
// the sums as words) with a lock and a completion event, so calls on one device serialise among themselves and with nothing else; the pairing workspace is not
// involved (an item here needs two field elements).  Launch sequence of one pass of m items (bn254_g1msm.h):
//   k_g1_msm_load -> k_g1_msm_rows (the handle's window tables) -> k_g1_sum_affine (words form) -> k_g1_msm_store
// Like bn254_capi_kzg.hip not part of the one-translation-unit host build of bn254_capi.hip: tests/hostsan/hostsan_g1_msm.cpp includes it itself, with
// bn254_capi_pairing.hip, whose host stream the host entry borrows.
#include "bn254_capi_internal.h"
#include "bn254_capi_pairing.h"
#include "bn254_g1msm.h"

static_assert(BN254_G1_MSM_MAX_VAR == G1MSM_MAX_VAR && BN254_G1_MSM_MAX_UNIT == G1MSM_MAX_UNIT && BN254_G1_MSM_MAX_SHARED == G1MSM_MAX_SHARED &&
              BN254_G1_MSM_ITEM_LEN(3, 1, 2) == G1MSM_ITEM_LEN(3, 1, 2) && BN254_G1_MSM_ITEM_LEN(1, 0, 0) == 96 && BN254_G1_MSM_ITEM_LEN(0, 2, 0) == 128,
              "the header's limits and item length are the loader's");
static_assert(G1MSM_BYTES_PER_ITEM(0, 0, 0) == 3522 && G1_GLV_TAB_BYTES_PER_LANE == 1792, "the pass formula of include/bn254_verify.h");

// the host entry stages a pass's items through pinned memory of at most this many bytes
#define G1M_STAGE_BYTES ((size_t)48 << 20)
#define G1M_BASES_MAGIC 0x42314742u      // "BG1B"

// device and pinned allocations of this unit so far (bn254_dbg_g1_msm_batch_state: "the device entry allocates nothing after the reserve")
static std::atomic<uint64_t> g_g1m_allocs{0};

// the handle of bn254_g1_bases_prepare: the window tables of its points on one device
struct G1Bases {
  uint32_t magic = G1M_BASES_MAGIC;
  int device = 0;
  size_t count = 0;
  uint32_t dead = 0;              // bit j: base j is the identity
  DevBuf<int32_t> tabs;           // count x MSM_FW_WINDOWS x MSM_FW_ENTRIES entries (bn254_fw.h)
};

namespace {

struct G1mDev {
  std::mutex mu;                  // (re)allocation and the enqueue of a call; held for the whole of a host-buffer call
  bool ready = false;
  Event busy_ev; bool busy_valid = false;
  DevBuf<int32_t> terms, part, glv; DevBuf<uint8_t> flags, st, inf; DevBuf<uint32_t> words;
  size_t part_points = 0, glv_lanes = 0;
  DevBuf<uint8_t> d_in, d_out; PinBuf<uint8_t> h_in, h_out;      // host entry: the items of a pass; its 64-byte results and, behind them, its status bytes
};
G1mDev* g1m_dev(int device) {      // never destroyed, map nodes never move (pb_dev)
  static std::mutex mu;
  static std::map<int, G1mDev>* devs = new std::map<int, G1mDev>();
  std::lock_guard<std::mutex> lk(mu);
  return &(*devs)[device];
}
template <class B> int g1m_grow(B& b, size_t n) {
  if (b && n <= b.cap()) return BN254_OK;
  g_g1m_allocs.fetch_add(1, std::memory_order_relaxed);
  return b.ensure(n);
}
// lack of memory, on the device or pinned, is BN254_E_NOMEM (the owners of bn254_capi_owners.h name the runtime's error in the message)
int g1m_rc(int rc) { return rc == BN254_E_HIP && g_err.find("out of memory") != std::string::npos ? set_err(BN254_E_NOMEM, std::string(g_err)) : rc; }

struct G1mCall {
  int v, u, s;
  const G1Bases* bases;
  bool strict;
  size_t lane_budget = 0; int joint_g = -1;      // the probe: the plan's form forced
  int n_terms() const { return v + u + s; }
  size_t item_len() const { return G1MSM_ITEM_LEN(v, u, s); }
};
size_t g1m_pass_items(const G1mCall& c) {
  static const size_t knob = bn254::knob_g1_msm_pass();
  const size_t m = bn254::g1msm_max_pass((size_t)c.v, (size_t)c.u, (size_t)c.s);
  return knob && knob < m ? knob : m;
}
bool g1m_plan(MsmPlan& plan, const G1mCall& c, size_t m_pad) {
  return msm_plan_build(plan, bn254::g1msm_shape(c.v, c.u, c.s), m_pad, c.lane_budget ? c.lane_budget : msm_lane_budget(), 0, c.joint_g >= 0 ? c.joint_g : plonk_joint_g(m_pad));
}
// caller holds d.mu.  The device ready (self-test at its first use) and the buffers grown to what launches of up to min(n, the items of a pass) items need; *launch: that many
int g1m_ensure(G1mDev& d, int device, size_t n, const G1mCall& c, size_t* launch) {
  int rc = check_device(device);
  if (rc || (rc = selftest_gate(device))) return rc;
  if (!d.ready) { if ((rc = d.busy_ev.ensure())) return rc; d.ready = true; }
  const size_t cap = g1m_pass_items(c), need = n < cap ? n : cap;
  *launch = need;
  const MsmShape sh = bn254::g1msm_shape(c.v, c.u, c.s);
  size_t lanes = plonk_scratch_lanes(need, c.v), points = plonk_part_points(need, sh);
  if (c.lane_budget || c.joint_g >= 0) {      // the probe's forced plan may take more rows than any launch the library plans
    MsmPlan plan;
    if (!g1m_plan(plan, c, (need + 63) & ~(size_t)63)) return set_err(BN254_E_BAD_ARG, "bad argument: the shape needs more MSM rows than a launch has");
    if (bn254_g1_msm_scratch_lanes(plan, need) > lanes) lanes = bn254_g1_msm_scratch_lanes(plan, need);
    if ((size_t)plan.n_rows * need > points) points = (size_t)plan.n_rows * need;
  }
  const size_t n_terms = (size_t)c.n_terms();
  if ((rc = g1m_grow(d.terms, need * n_terms * MSM_TERM_DWORDS)) || (rc = g1m_grow(d.flags, need * n_terms)) || (rc = g1m_grow(d.st, need)) || (rc = g1m_grow(d.inf, need)) ||
      (rc = g1m_grow(d.words, need * 16)))
    return rc;
  if (points > d.part_points) { d.part_points = 0; if ((rc = g1m_grow(d.part, points * 27))) return rc; d.part_points = points; }
  // (a shape without variable terms still gets a lane: the launcher is handed a pointer it may look at)
  if (lanes > d.glv_lanes || !d.glv) { d.glv_lanes = 0; if ((rc = g1m_grow(d.glv, (lanes ? lanes : 1) * (size_t)(G1_GLV_TAB_BYTES_PER_LANE / 4)))) return rc; d.glv_lanes = lanes; }
  return BN254_OK;
}

// One launch of m items, everything on s; caller holds d.mu and has run g1m_ensure.  d_out / d_status: 64 m and m bytes of the caller's.  info: null or the probe's six values
int g1m_launch(G1mDev& d, const G1mCall& c, const uint8_t* d_items, size_t stride, size_t m, uint8_t* d_out, uint8_t* d_status, hipStream_t s, int* info) {
  const size_t m_pad = (m + 63) & ~(size_t)63, n_terms = (size_t)c.n_terms();
  MsmPlan plan;
  if (!g1m_plan(plan, c, m_pad)) return set_err(BN254_E_HIP, "G1 MSM: the walk needs more rows than a launch has");
  if (m > G1MSM_MAX_PASS || bn254_g1_msm_scratch_lanes(plan, m) > d.glv_lanes || (size_t)plan.n_rows * m > d.part_points || d.terms.cap() < m * n_terms * MSM_TERM_DWORDS ||
      d.flags.cap() < m * n_terms || d.st.cap() < m || d.inf.cap() < m || d.words.cap() < 16 * m)
    return set_err(BN254_E_HIP, "G1 MSM buffers smaller than the launch (internal sizing error)");
  if (info) {
    bool split = false, joint = false;
    for (int r = 0; r < plan.n_rows; r++) { joint |= plan.row[r].n_joint != 0; split |= plan.row[r].var_term >= 0 && (plan.row[r].pos_lo != 0 || plan.row[r].pos_hi != 128); }
    info[0] = plan.n_rows; info[1] = plan.n_var_rows; info[2] = plan.count[0]; info[3] = plan.count[1]; info[4] = joint ? 2 : split ? 0 : 1; info[5] = msm_plan_chain(plan);
  }
  bn254::G1MsmLoadArgs a;
  a.items = d_items; a.stride = stride; a.n = m; a.n_var = c.v; a.n_unit = c.u; a.n_shared = c.s; a.dead_bases = c.bases ? c.bases->dead : 0u; a.strict = c.strict;
  a.status = d.st; a.terms = d.terms; a.flags = d.flags;
  hipError_t e = bn254_launch_g1msm_load(a, s);
  // without a shared term the table pointer is never read (any device address)
  if (e == hipSuccess) e = bn254_launch_g1_msm_rows(plan, d.terms, d.flags, m, (int)n_terms, d.part, d.glv, c.s ? (const int32_t*)c.bases->tabs : (const int32_t*)d.terms, s);
  if (e == hipSuccess) e = bn254_launch_g1_sum_rows(plan, d.part, m, d.words, d.inf, nullptr, nullptr, 0, 0, 0, 0, s);
  if (e == hipSuccess) e = bn254_launch_g1msm_store(d.words, d.inf, d.st, m, d_out, d_status, s);
  if (e != hipSuccess) return launch_err(e, "G1 MSM");
  return BN254_OK;
}
// the launches of a call on device memory: caller holds d.mu
int g1m_enqueue(G1mDev& d, const G1mCall& c, const uint8_t* d_items, size_t stride, size_t n, uint8_t* d_out, uint8_t* d_status, size_t launch, hipStream_t s, int* info = nullptr) {
  if (d.busy_valid) HIPCK(hipStreamWaitEvent(s, d.busy_ev, 0));
  int rc = BN254_OK;
  for (size_t off = 0; off < n && !rc; off += launch)
    rc = g1m_launch(d, c, d_items + off * stride, stride, n - off < launch ? n - off : launch, d_out + 64 * off, d_status + off, s, info);
  // also after a failure: whatever was enqueued must be behind the event the next call waits for
  const hipError_t e = hipEventRecord(d.busy_ev, s);
  if (e == hipSuccess) d.busy_valid = true;
  if (!rc && e != hipSuccess) return set_err(BN254_E_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
  return rc;
}

// BN254_E_BAD_ARG before any device is touched; *done: n == 0
int g1m_check_args(const void* items, size_t stride, size_t v, size_t u, size_t s, const void* bases, size_t n, const void* out, const void* status, int device, unsigned flags, bool* done,
                   bool raw_bases = false /* the probe: the bases come as points, not as a handle */) {
  *done = false;
  if (flags & ~(unsigned)BN254_FLAG_STRICT_SCALARS) return set_err(BN254_E_BAD_ARG, "bad argument: flags other than BN254_FLAG_STRICT_SCALARS");
  if (!bn254::g1msm_shape_ok(v, u, s)) return set_err(BN254_E_BAD_ARG, "bad argument: the shape is 0 .. 16 variable, 0 .. 4 unit and 0 .. 16 shared terms, one at least");
  if (stride < G1MSM_ITEM_LEN(v, u, s)) return set_err(BN254_E_BAD_ARG, "bad argument: item_stride below BN254_G1_MSM_ITEM_LEN(n_var, n_unit, n_shared)");
  const G1Bases* b = (const G1Bases*)bases;
  if (s && !b && !raw_bases) return set_err(BN254_E_BAD_ARG, "bad argument: shared terms without a bases handle");
  if (b && b->magic != G1M_BASES_MAGIC) return set_err(BN254_E_BAD_ARG, "bad argument: not a handle of bn254_g1_bases_prepare");
  if (b && s > b->count) return set_err(BN254_E_BAD_ARG, "bad argument: n_shared above the handle's count");
  if (b && b->device != device) return set_err(BN254_E_BAD_ARG, "bad argument: the bases handle belongs to another device");
  if (n && (!items || !out || !status)) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n && stride > SIZE_MAX / n) return set_err(BN254_E_BAD_ARG, "bad argument: n items of item_stride bytes overflow the address space");
  *done = n == 0;
  return BN254_OK;
}

// a host-buffer call: passes through pinned staging (the items packed, padded to whole dwords); info: the probe's, which takes one pass
int g1m_host_call(const G1mCall& c, const uint8_t* items, size_t stride, size_t n, uint8_t* out, uint8_t* status, int device, int* info) {
  G1mDev* d = g1m_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  const size_t ilen = c.item_len(), slen = (ilen + 3) & ~(size_t)3;
  size_t launch = 0;
  int rc;
  if ((rc = g1m_ensure(*d, device, n, c, &launch))) return rc;
  // The host entry runs on the stream of the pairing batch's host entries, not on one of its own: every stream of a process takes a share of the runtime's few
  // hardware queues (DevState::aux has the measurement), and one more library stream was enough to put the sub-batch streams of a Groth16 key on one queue.  Only
  // the stream is shared -- created under its owner's lock, never destroyed -- the buffers and the lock are this entry's
  hipStream_t s;
  {
    PbDev* pd = pb_dev(device);
    std::lock_guard<std::mutex> plk(pd->mu);
    if ((rc = pd->stream.ensure())) return rc;
    s = pd->stream;
  }
  size_t pass = G1M_STAGE_BYTES / slen;
  if (pass > launch) pass = launch;
  if (info && n > pass) return set_err(BN254_E_BAD_ARG, "bad argument: the probe takes one pass");
  if ((rc = g1m_grow(d->h_in, pass * slen)) || (rc = g1m_grow(d->d_in, pass * slen)) || (rc = g1m_grow(d->h_out, pass * 65)) || (rc = g1m_grow(d->d_out, pass * 65))) return rc;
  auto one_pass = [&](size_t off, size_t m) -> int {
    uint8_t* o = d->h_in;
    if (stride == ilen && ilen == slen) parallel_copy(o, items + off * stride, m * slen);
    else for (size_t i = 0; i < m; i++) memcpy(o + i * slen, items + (off + i) * stride, ilen);
    HIPCK(hipMemcpyAsync(d->d_in, d->h_in, m * slen, hipMemcpyHostToDevice, s));
    int r = g1m_enqueue(*d, c, d->d_in, slen, m, d->d_out, d->d_out + 64 * pass, launch, s, info);
    if (r) return r;
    HIPCK(hipMemcpyAsync(d->h_out, d->d_out, 64 * m, hipMemcpyDeviceToHost, s));
    HIPCK(hipMemcpyAsync(d->h_out + 64 * pass, d->d_out + 64 * pass, m, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    memcpy(out + 64 * off, d->h_out, 64 * m);
    memcpy(status + off, d->h_out + 64 * pass, m);
    return BN254_OK;
  };
  for (size_t off = 0; off < n; off += pass) {
    if ((rc = one_pass(off, n - off < pass ? n - off : pass))) {
      const std::string keep = g_err;      // the staging must be quiescent when the lock is released
      (void)hipStreamSynchronize(s);
      return set_err(rc, keep);
    }
  }
  return BN254_OK;
}

// the checks of bn254_g1_bases_prepare on n_bases points: *status, and (ACCEPT) the points as digits -- an identity base as the generator, whose table stands in for
// one that is never consulted -- and the identity bits
int g1m_parse_bases(const uint8_t* points, size_t n_bases, std::vector<int32_t>& pts, std::vector<bn254::G1Aff>& aff, uint32_t* dead, uint8_t* status) {
  pts.assign(n_bases * 2 * BN_NL, 0); aff.resize(n_bases); *dead = 0;
  for (size_t j = 0; j < n_bases; j++) {
    bool memb = true, zero = true;
    bn254::G1Aff p = bn254::g1msm_point(points + 64 * j, false, memb, zero);
    if (!memb) { *status = BN254_ERR_NOT_MEMBER; return BN254_OK; }
    if (!zero && !bn254::g1_on_curve(p)) { *status = BN254_ERR_NOT_ON_CURVE; return BN254_OK; }
    if (zero) { *dead |= 1u << j; uint32_t w[8] = {1, 0, 0, 0, 0, 0, 0, 0}; p.x = bn254::fp_from_words(w); w[0] = 2; p.y = bn254::fp_from_words(w); }
    aff[j] = p;
    fp_to_limbs(pts.data() + j * 2 * BN_NL, p.x); fp_to_limbs(pts.data() + j * 2 * BN_NL + BN_NL, p.y);
  }
  *status = BN254_ACCEPT;
  return BN254_OK;
}
int g1m_bases_make(const uint8_t* points, size_t n_bases, int device, G1Bases** out, uint8_t* status) {
  *out = nullptr;
  std::vector<int32_t> pts; std::vector<bn254::G1Aff> aff; uint32_t dead;
  int rc = g1m_parse_bases(points, n_bases, pts, aff, &dead, status);
  if (rc || *status != BN254_ACCEPT) return rc;
  if ((rc = check_device(device)) || (rc = selftest_gate(device))) return rc;
  std::unique_ptr<G1Bases> b(new G1Bases());
  b->device = device; b->count = n_bases; b->dead = dead;
  if ((rc = build_tables_on_device(2, pts, b->tabs))) return g1m_rc(rc);
  *out = b.release();
  return BN254_OK;
}
void g1m_bases_drop(G1Bases* b) {
  if (!b || b->magic != G1M_BASES_MAGIC) return;
  // the launches that read the tables were enqueued on the callers' streams: wait for the device before the memory goes
  if (hipSetDevice(b->device) == hipSuccess) (void)hipDeviceSynchronize();
  b->magic = 0;
  delete b;
}

// ---- the host compile: the loader, the rows of the plan, the row sum and the store on plain arrays (bn254_dbg_g1_msm_batch with device -1) --------------------------
// entry (w, d) of base j's window table, (d + 1) 2^(MSM_FW_BITS w) B_j, made when first asked for
struct G1mHostTabs {
  std::vector<bn254::G1Proj> win;      // 2^(MSM_FW_BITS w) B_j at j * MSM_FW_WINDOWS + w
  mutable std::map<uint64_t, bn254::G1Aff> memo;
  explicit G1mHostTabs(const std::vector<bn254::G1Aff>& bases) : win(bases.size() * MSM_FW_WINDOWS) {
    for (size_t j = 0; j < bases.size(); j++) {
      bn254::G1Proj p = bn254::g1_from_affine(bases[j]);
      for (int w = 0; w < (int)MSM_FW_WINDOWS; w++) {
        win[j * MSM_FW_WINDOWS + w] = p;
        for (int k = 0; k < MSM_FW_BITS; k++) { p = bn254::g1_dbl(p); p.x = bn254::fp_reduce(p.x); p.y = bn254::fp_reduce(p.y); p.z = bn254::fp_reduce(p.z); }
      }
    }
  }
  bn254::G1Aff entry(int tab, int w, uint32_t d) const {
    const uint64_t key = ((uint64_t)tab << 40) | ((uint64_t)w << 32) | d;
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
    const bn254::G1Proj b = win[(size_t)tab * MSM_FW_WINDOWS + w];
    bn254::G1Proj acc = bn254::g1_identity();
    for (int bit = MSM_FW_BITS; bit >= 0; bit--) {
      acc = bn254::g1_dbl(acc);
      if (((d + 1) >> bit) & 1u) acc = bn254::g1_add(acc, b);
      acc.x = bn254::fp_reduce(acc.x); acc.y = bn254::fp_reduce(acc.y); acc.z = bn254::fp_reduce(acc.z);
    }
    bn254::G1Aff a = bn254::g1_to_affine(acc);
    a.x = bn254::fp_reduce(bn254::fp_norm(a.x)); a.y = bn254::fp_reduce(bn254::fp_norm(a.y));
    memo[key] = a;
    return a;
  }
};
struct G1mHostIO {      // DevMsmIO on host arrays
  const int32_t* t; const uint8_t* f; const G1mHostTabs* tabs;
  void term(int q, bn254::G1Aff& P, uint32_t k1[4], uint32_t k2[4], uint32_t& fl) const {
    const int32_t* e = t + (size_t)q * MSM_TERM_DWORDS;
    for (int l = 0; l < BN_NL; l++) { P.x.v[l] = e[l]; P.y.v[l] = e[BN_NL + l]; }
    BN_SETB(P.x, 1.0, 0.5); BN_SETB(P.y, 1.0, 0.5);
    for (int w = 0; w < 4; w++) { k1[w] = (uint32_t)e[18 + w]; k2[w] = (uint32_t)e[22 + w]; }
    fl = f[q];
  }
  uint32_t kword(int q, int half, int w) const { return (uint32_t)t[(size_t)q * MSM_TERM_DWORDS + 18 + 4 * half + w]; }
  uint32_t scalar_digit(int q, int w) const {
    const int32_t* k = t + (size_t)q * MSM_TERM_DWORDS + 18;
    const int bit = MSM_FW_BITS * w, i = bit >> 5, sh = bit & 31;
    const uint64_t two = (uint64_t)(uint32_t)k[i] | ((uint64_t)(i + 1 < 8 ? (uint32_t)k[i + 1] : 0u) << 32);
    return (uint32_t)(two >> sh) & MSM_FW_ENTRIES;
  }
  bn254::G1Aff entry(int tab, int w, uint32_t d) const { return tabs->entry(tab, w, d); }
};
struct G1mHostTab {
  bn254::G1Proj* t;
  void put(int i, const bn254::G1Proj& p) { t[i].x = bn254::fp_reduce(p.x); t[i].y = bn254::fp_reduce(p.y); t[i].z = bn254::fp_reduce(p.z); }
  bn254::G1Proj get(uint32_t i) const { return t[i]; }
  void fence() {}
  G1mHostTab slot(int j) const { return G1mHostTab{t + 16 * j}; }
};
int g1m_on_host(const G1mCall& c, const uint8_t* items, size_t stride, const uint8_t* base_points, size_t n_bases, size_t n, uint8_t* out, uint8_t* status, int* info) {
  using namespace bn254;
  std::vector<int32_t> pts; std::vector<G1Aff> aff; uint32_t dead = 0; uint8_t bst = BN254_ACCEPT;
  if (n_bases) { const int rc = g1m_parse_bases(base_points, n_bases, pts, aff, &dead, &bst); if (rc) return rc; }
  if (bst != BN254_ACCEPT) return set_err(BN254_E_BAD_ARG, "bad argument: a base is not a curve point");
  const G1mHostTabs tabs(aff);
  const size_t n_pad = (n + 63) & ~(size_t)63;
  MsmPlan plan;
  if (!g1m_plan(plan, c, n_pad)) return set_err(BN254_E_BAD_ARG, "bad argument: the shape needs more MSM rows than a launch has");
  if (info) {
    bool split = false, joint = false;
    for (int r = 0; r < plan.n_rows; r++) { joint |= plan.row[r].n_joint != 0; split |= plan.row[r].var_term >= 0 && (plan.row[r].pos_lo != 0 || plan.row[r].pos_hi != 128); }
    info[0] = plan.n_rows; info[1] = plan.n_var_rows; info[2] = plan.count[0]; info[3] = plan.count[1]; info[4] = joint ? 2 : split ? 0 : 1; info[5] = msm_plan_chain(plan);
  }
  const int n_terms = c.n_terms();
  std::vector<int32_t> terms((size_t)n_terms * MSM_TERM_DWORDS);
  std::vector<uint8_t> fl(n_terms);
  std::vector<G1Proj> store(16 * MSM_MAX_JOINT);
  for (size_t i = 0; i < n; i++) {
    const int st = g1msm_load_item(items + i * stride, false, c.v, c.u, c.s, dead, c.strict, terms.data(), fl.data());
    G1mHostIO io{terms.data(), fl.data(), &tabs};
    G1Proj L = g1_identity();      // k_g1_sum_affine, one lane per item
    for (int r = plan.first[0]; r < plan.first[0] + plan.count[0]; r++) {
      G1mHostTab tab{store.data()};
      G1Proj row = msm_row_eval(plan, r, io, tab);
      BN_SETB(row.x, 3.0, 0.5); BN_SETB(row.y, 3.0, 0.5); BN_SETB(row.z, 3.0, 0.5);
      L = g1_add(L, row);
    }
    const bool inf = g1_is_identity(L);
    const G1Aff a = g1_to_affine(L);
    uint32_t w16[16];
    fp_to_words(w16, a.x); fp_to_words(w16 + 8, a.y);
    g1msm_store_item(out + 64 * i, status + i, st, w16, inf, false);
  }
  return BN254_OK;
}

}  // namespace

extern "C" {

int bn254_g1_bases_prepare(const uint8_t* points, size_t n_bases, int device, void** out, uint8_t* status) {
  if (out) *out = nullptr;
  if (!points || !out || !status || n_bases < 1 || n_bases > (size_t)G1MSM_MAX_SHARED) return set_err(BN254_E_BAD_ARG, "bad argument: 1 .. BN254_G1_MSM_MAX_SHARED points");
  G1Bases* b = nullptr;
  const int rc = g1m_bases_make(points, n_bases, device, &b, status);
  *out = b;
  return rc;
}
void bn254_g1_bases_free(void* bases) { g1m_bases_drop((G1Bases*)bases); }
size_t bn254_g1_bases_count(const void* bases) {
  const G1Bases* b = (const G1Bases*)bases;
  return b && b->magic == G1M_BASES_MAGIC ? b->count : 0;
}

int bn254_g1_msm_reserve(size_t n, size_t n_var, size_t n_unit, size_t n_shared, int device) {
  if (!bn254::g1msm_shape_ok(n_var, n_unit, n_shared)) return set_err(BN254_E_BAD_ARG, "bad argument: the shape is 0 .. 16 variable, 0 .. 4 unit and 0 .. 16 shared terms, one at least");
  const G1mCall c{(int)n_var, (int)n_unit, (int)n_shared, nullptr, false};
  G1mDev* d = g1m_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  size_t launch;
  return g1m_rc(g1m_ensure(*d, device, n ? n : 1, c, &launch));
}

int bn254_g1_msm_batch(const uint8_t* items, size_t item_stride, size_t n_var, size_t n_unit, size_t n_shared, const void* bases, size_t n, uint8_t* out, uint8_t* status, int device,
                       unsigned flags) {
  bool done;
  const int rc = g1m_check_args(items, item_stride, n_var, n_unit, n_shared, bases, n, out, status, device, flags, &done);
  if (rc || done) return rc;
  const G1mCall c{(int)n_var, (int)n_unit, (int)n_shared, (const G1Bases*)bases, (flags & BN254_FLAG_STRICT_SCALARS) != 0};
  return g1m_rc(g1m_host_call(c, items, item_stride, n, out, status, device, nullptr));
}

int bn254_g1_msm_batch_device(const void* d_items, size_t item_stride, size_t n_var, size_t n_unit, size_t n_shared, const void* bases, size_t n, void* d_out, void* d_status,
                              int device, void* hip_stream, unsigned flags) {
  bool done;
  int rc = g1m_check_args(d_items, item_stride, n_var, n_unit, n_shared, bases, n, d_out, d_status, device, flags, &done);
  if (rc || done) return rc;
  const G1mCall c{(int)n_var, (int)n_unit, (int)n_shared, (const G1Bases*)bases, (flags & BN254_FLAG_STRICT_SCALARS) != 0};
  G1mDev* d = g1m_dev(device);
  std::lock_guard<std::mutex> lk(d->mu);
  // nothing is allocated when a reservation (or an earlier call) of min(n, the items of a pass) items of this shape stands
  size_t launch;
  if ((rc = g1m_ensure(*d, device, n, c, &launch))) return g1m_rc(rc);
  return g1m_rc(g1m_enqueue(*d, c, (const uint8_t*)d_items, item_stride, n, (uint8_t*)d_out, (uint8_t*)d_status, launch, (hipStream_t)hip_stream));
}

// The probe: one pass with the plan's form forced (lane_budget 0: the library's; 64: the unsplit form at any n; joint_g -1: the library's rule, 0 / 1 none, 2 .. 8 joint
// rows in an unsplit launch), the bases as raw points (n_bases >= n_shared; may be 0 without shared terms).  info: rows, variable rows, rows of the sum, 0, the form
// (0 split, 1 unsplit, 2 joint), the longest row in the planner's units.  device -1: the host compile of the loader body, the planned rows, the row sum and the store,
// window-table entries made on the host; a device ordinal: the kernels, through the host-buffer path
int bn254_dbg_g1_msm_batch(const uint8_t* items, size_t item_stride, size_t n_var, size_t n_unit, size_t n_shared, const uint8_t* base_points, size_t n_bases, size_t n, unsigned flags,
                           size_t lane_budget, int joint_g, uint8_t* out, uint8_t* status, int info[6], int device) {
  if (!info || n_bases > (size_t)G1MSM_MAX_SHARED || n_shared > n_bases || (n_bases && !base_points) || (lane_budget && lane_budget < 64) || joint_g < -1 || joint_g > MSM_MAX_JOINT ||
      device < -1)
    return set_err(BN254_E_BAD_ARG, "bad argument: lane_budget is 0 or at least 64, joint_g -1 .. 8, n_shared at most n_bases");
  bool done;
  int rc = g1m_check_args(items, item_stride, n_var, n_unit, n_shared, nullptr, n, out, status, device, flags, &done, true);
  if (rc || done) return rc;
  G1mCall c{(int)n_var, (int)n_unit, (int)n_shared, nullptr, (flags & BN254_FLAG_STRICT_SCALARS) != 0};
  c.lane_budget = lane_budget; c.joint_g = joint_g;
  if (device < 0) return g1m_on_host(c, items, item_stride, base_points, n_bases, n, out, status, info);
  G1Bases* b = nullptr;
  if (n_bases) {
    uint8_t bst = BN254_ACCEPT;
    if ((rc = g1m_bases_make(base_points, n_bases, device, &b, &bst))) return rc;
    if (bst != BN254_ACCEPT) return set_err(BN254_E_BAD_ARG, "bad argument: a base is not a curve point");
  }
  c.bases = b;
  rc = g1m_rc(g1m_host_call(c, items, item_stride, n, out, status, device, info));
  const std::string keep = g_err;
  g1m_bases_drop(b);
  return rc ? set_err(rc, keep) : rc;
}
// whether the walk of n items of a shape plans, and its rows (bn254_dbg_kzg_fold_plan for this entry); host only
int bn254_dbg_g1_msm_batch_plan(size_t n_var, size_t n_unit, size_t n_shared, size_t n, size_t lane_budget, int joint_g, int* rows) {
  if (n_var > (size_t)MSM_MAX_FIXED || n_unit > 4 || n_shared > (size_t)MSM_MAX_FIXED || n == 0) return set_err(BN254_E_BAD_ARG, "bad argument");
  G1mCall c{(int)n_var, (int)n_unit, (int)n_shared, nullptr, false};
  c.lane_budget = lane_budget; c.joint_g = joint_g;
  MsmPlan plan;
  if (!g1m_plan(plan, c, (n + 63) & ~(size_t)63)) return set_err(BN254_E_BAD_ARG, "shape cannot be planned");
  if (rows) *rows = plan.n_rows;
  return BN254_OK;
}
// {items of a pass for the shape under BN254_G1_MSM_PASS, the formula's bound, the formula's bytes per item, allocations of this unit so far}
int bn254_dbg_g1_msm_batch_state(size_t n_var, size_t n_unit, size_t n_shared, uint64_t out[4]) {
  if (!out || !bn254::g1msm_shape_ok(n_var, n_unit, n_shared)) return set_err(BN254_E_BAD_ARG, "bad argument");
  const G1mCall c{(int)n_var, (int)n_unit, (int)n_shared, nullptr, false};
  out[0] = g1m_pass_items(c); out[1] = bn254::g1msm_max_pass(n_var, n_unit, n_shared); out[2] = G1MSM_BYTES_PER_ITEM(n_var, n_unit, n_shared);
  out[3] = g_g1m_allocs.load(std::memory_order_relaxed);
  return BN254_OK;
}

}  // extern "C"
