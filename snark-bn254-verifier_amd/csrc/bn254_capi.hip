// bn254_capi.hip -- implementation of the C ABI declared in include/bn254_verify.h: version, errors and status strings, the host plumbing the
// protocol files share, the point codecs and the SP1 fixture parser, the shard plan and the status all-gather of multi-device jobs.
// The protocols live beside it: bn254_capi_g16.hip (Groth16), bn254_capi_plonk.hip (PlonK), bn254_capi_sp1.hip (SP1 proofs from their public values),
// bn254_capi_dbg.hip (test probes, workload generator), bn254_capi_selftest.hip (the device self-test and its gate).
// Host orchestration only: key preparation (bn254_host.hpp), device buffers, kernel launches (the launchers of the kernel units, bn254_kernels.h).
// There is deliberately no CPU implementation of verify here: if HIP is unusable the calls fail (BN254_E_NO_DEVICE).
#if !defined(__HIPCC__)
#define BN254_SELFTEST_TABLES 1      // the one-unit host build (bottom of this file) brings bn254_capi_selftest.hip, which reads the tables of bn254_constants.h
#endif
#include "bn254_capi_internal.h"

static_assert(BN254_REJECT == BN254_ST_REJECT && BN254_ACCEPT == BN254_ST_ACCEPT && BN254_ERR_NOT_MEMBER == BN254_ST_NOT_MEMBER &&
              BN254_ERR_NOT_ON_CURVE == BN254_ST_NOT_ON_CURVE && BN254_ERR_NOT_IN_SUBGROUP == BN254_ST_NOT_IN_SUBGROUP &&
              BN254_ERR_INPUT_LEN == BN254_ST_INPUT_LEN && BN254_ERR_MALFORMED == BN254_ST_MALFORMED, "status codes out of sync");

thread_local std::string g_err;
int set_err(int code, const std::string& msg) { g_err = msg; return code; }
// The argument check every Groth16 and PlonK batch entry makes first, before it touches a device or computes a size.  Groth16 records hold
// at least the 256-byte raw proof and know BN254_FLAG_RLC | BN254_FLAG_STRICT_SCALARS; PlonK records are judged by the parser and know BN254_FLAG_RLC.
// Beyond the pointers and flags: n records of proof_stride + 32 n_public bytes must be addressable (a key without K points reports SIZE_MAX public
// inputs, bn254_groth16_vk_num_public, and n * row would wrap).
int check_batch_args(bool plonk, const void* pvk, const void* proofs, size_t proof_stride, const void* inputs, size_t n_public, size_t n, const void* status,
                     unsigned flags) {
  // Groth16: raw records of >= 256 bytes, or with BN254_FLAG_COMPRESSED_PROOFS gnark's compressed records of >= 128 bytes
  const size_t min_stride = (!plonk && (flags & BN254_FLAG_COMPRESSED_PROOFS)) ? 128 : 256;
  if (!pvk || (n && (!proofs || !status)) || (n && n_public && !inputs) || (!plonk && (proof_stride < min_stride || (flags & ~7u)))) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (plonk && (flags & ~(unsigned)BN254_FLAG_RLC)) return set_err(BN254_E_BAD_ARG, "unknown flag (the PlonK batch entry knows BN254_FLAG_RLC)");
  if (n && (n_public > (SIZE_MAX - proof_stride) / 32 || proof_stride + 32 * n_public > SIZE_MAX / n))
    return set_err(BN254_E_BAD_ARG, "n_public too large: n records of proof_stride + 32 n_public bytes overflow the address space");
  return BN254_OK;
}

int check_key_list(const bn254_g16_pvk* const* pvks, size_t n_keys, size_t* max_public) {
  if (!pvks || n_keys == 0) return set_err(BN254_E_BAD_ARG, "bad argument: empty key list");
  if (n_keys > (size_t)G16_KEYS_MAX_KEYS) {
    set_diag("a key list holds at most " + std::to_string(G16_KEYS_MAX_KEYS) + " entries (got " + std::to_string(n_keys) + ")");
    return set_err(BN254_E_BAD_ARG, "key list too long");
  }
  size_t mx = 0;
  for (size_t k = 0; k < n_keys; k++) {
    if (!pvks[k]) return set_err(BN254_E_BAD_ARG, "bad argument: null key in the list");
    const size_t ki = pvks[k]->host.key_inputs();
    if (ki > (size_t)G16_KEYS_MAX_PUBLIC) {
      set_diag("entry " + std::to_string(k) + " of the key list has " + std::to_string(ki) + " public inputs: batches over many keys take keys with up to " +
               std::to_string(G16_KEYS_MAX_PUBLIC) + " (wider keys run the wide MSM kernels: one call per key, bn254_groth16_verify_batch)");
      return set_err(BN254_E_BAD_ARG, "a key of the list has more than 16 public inputs");
    }
    if (ki > mx) mx = ki;
  }
  *max_public = mx;
  return BN254_OK;
}
int check_keys_args(const bn254_g16_pvk* const* pvks, size_t n_keys, const void* key_index, const void* proofs, size_t proof_stride, const void* inputs, size_t input_stride,
                    size_t n, const void* status, unsigned flags, size_t* max_public) {
  int rc = check_key_list(pvks, n_keys, max_public);
  if (rc) return rc;
  // records, status and flags as in every Groth16 batch entry (the input rows are checked below: their width is the list's, not an argument)
  if ((rc = check_batch_args(false, pvks, proofs, proof_stride, nullptr, 0, n, status, flags))) return rc;
  if (n && !key_index) return set_err(BN254_E_BAD_ARG, "bad argument: null key index");
  if (input_stride < 32 * *max_public) return set_err(BN254_E_BAD_ARG, "input_stride is smaller than the inputs of the widest key of the list (32 bytes each)");
  if (n && *max_public && !inputs) return set_err(BN254_E_BAD_ARG, "bad argument: null public inputs");
  if (n && (input_stride > SIZE_MAX / n || bn254::keys_slot_bound(n, n_keys) > 0xffff0000ull)) return set_err(BN254_E_BAD_ARG, "batch too large: slots and input rows are addressed with 32 / 64 bits");
  return BN254_OK;
}

int check_device(int device) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0) return set_err(BN254_E_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= cnt) return set_err(BN254_E_BAD_ARG, "device ordinal out of range");
  HIPCK(hipSetDevice(device));
  return BN254_OK;
}
// The fixed-base tables of a key, built on the current device from the key's points (bn254_k_comb.hip; form 0: comb tables, 1: byte windows; pts: 18 dwords per point):
// 80 bytes x 8192 (8160) entries per point stay, the construction scratch (27 dwords per entry, passes of 256 points: 226 MB at most) is freed again.  *dst stays null unless
// the table is complete (as upload(), bn254_capi_internal.h).
int build_tables_on_device(int form, const std::vector<int32_t>& pts, DevBuf<int32_t>& dst) {
  if (dst) return BN254_OK;
  const size_t np = pts.size() / (2 * BN_NL);
  const size_t per_point = bn254_tab_build_out_entries(form) * MSM_ENTRY_DWORDS;   // dwords of finished table per point
  const size_t teeth = bn254_tab_build_teeth(form), entries = bn254_tab_build_entries(form);
  const size_t slice_cap = ((size_t)256 << 13) / entries ? ((size_t)256 << 13) / entries : 1;   // points per pass: 2 M construction entries (226 MB of scratch) at most
  const size_t slice = np < slice_cap ? np : slice_cap;
  DevBuf<int32_t> kp, tab, tplane, taff, plane;     // the scratch goes when this function returns
  int rc;
  if ((rc = kp.ensure(pts.size())) || (rc = tab.ensure(np * per_point)) || (rc = tplane.ensure(slice * teeth * 27)) || (rc = taff.ensure(slice * teeth * 2 * BN_NL)) ||
      (rc = plane.ensure(slice * entries * 27)))
    return rc;
  hipError_t e = hipMemcpy(kp, pts.data(), pts.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  for (size_t i0 = 0; i0 < np && e == hipSuccess; i0 += slice) {
    const size_t m = np - i0 < slice ? np - i0 : slice;            // the passes run one after the other on the null stream and share the scratch
    e = bn254_launch_tab_build(form, kp + i0 * 2 * BN_NL, (uint32_t)m, tab + i0 * per_point, tplane, taff, plane, nullptr);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("fixed-base tables of the key: ") + hipGetErrorString(e));
  dst = std::move(tab);
  return BN254_OK;
}
// BN254_STREAMS = 1..4 sub-batches of a Groth16 chunk in flight (default 2: +4.5 % over one stream at 2^20, profiles/r01_streams.txt); a key set runs at most two
int sub_batch_streams() {
  static const int n = [] { const char* e = getenv("BN254_STREAMS"); int v = e ? atoi(e) : 2; return v < 1 ? 1 : (v > 4 ? 4 : v); }();
  return n;
}
// Host threads of the staging copies (parallel_copy): one process-wide pool, started on first use.  (Spawning and joining 16 threads costs ~0.4 ms,
// 8 % of a 4096-proof batch.)  run(n, fn) executes fn(0) on the caller and fn(1..n-1) on pool threads and returns when all
// are done; jobs of concurrent callers (the sub-batch workers of a large batch, other keys) share the queue.
class HostPool {
 public:
  static HostPool& get() {
    static HostPool pool([] { unsigned hw = std::thread::hardware_concurrency(); if (hw == 0) hw = 1; return hw > 32 ? 32u : hw; }());
    return pool;
  }
  void run(unsigned n, const std::function<void(unsigned)>& fn) {
    if (n <= 1) { fn(0); return; }
    struct Job { std::mutex m; std::condition_variable c; unsigned left; bool failed = false; } job;
    job.left = n - 1;
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (unsigned t = 1; t < n; t++)
        q_.emplace_back([&job, &fn, t] {
          try { fn(t); } catch (...) { std::lock_guard<std::mutex> l(job.m); job.failed = true; }   // a pool thread must not die with the job still counted
          std::lock_guard<std::mutex> l(job.m);
          if (--job.left == 0) job.c.notify_one();
        });
    }
    cv_.notify_all();
    // the queued lambdas reference `job` and `fn` on this frame: whatever fn(0) does -- including throwing -- the frame must outlive them
    struct Wait {
      Job& j;
      ~Wait() { std::unique_lock<std::mutex> lk(j.m); j.c.wait(lk, [this] { return j.left == 0; }); }
    } wait{job};
    fn(0);
    {
      std::unique_lock<std::mutex> lk(job.m);
      job.c.wait(lk, [&] { return job.left == 0; });
      if (job.failed) throw std::runtime_error("a host-pool slice failed");
    }
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }

 private:
  explicit HostPool(unsigned n) { for (unsigned i = 0; i < n; i++) th_.emplace_back([this] { loop(); }); }
  void loop() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;
        f = std::move(q_.front()); q_.pop_front();
      }
      f();
    }
  }
  std::mutex mu_; std::condition_variable cv_; std::deque<std::function<void()>> q_; std::vector<std::thread> th_; bool stop_ = false;
};
void parallel_copy(uint8_t* dst, const uint8_t* src, size_t bytes) {
  static const unsigned hw = [] { unsigned v = std::thread::hardware_concurrency(); const char* e = getenv("BN254_HOST_COPY_THREADS"); if (e) v = (unsigned)atoi(e); return v < 1 ? 1u : (v > 8 ? 8u : v); }();
  if (bytes < ((size_t)4 << 20) || hw == 1) { memcpy(dst, src, bytes); return; }
  const size_t per = ((bytes + hw - 1) / hw + 4095) & ~(size_t)4095;
  HostPool::get().run(hw, [&](unsigned t) {
    const size_t lo = (size_t)t * per;
    if (lo < bytes) memcpy(dst + lo, src + lo, bytes - lo < per ? bytes - lo : per);
  });
}

extern "C" {

const char* bn254_last_error(void) { return g_err.c_str(); }
const char* bn254_version(void) { return "bn254-verify-amd 0.5 (gfx950)"; }
int bn254_abi_version(void) { return BN254_ABI_VERSION; }
const char* bn254_status_string(int s) {
  switch (s) {
    case BN254_REJECT: return "reject"; case BN254_ACCEPT: return "accept"; case BN254_ERR_NOT_MEMBER: return "coordinate not a field member";
    case BN254_ERR_NOT_ON_CURVE: return "point not on curve"; case BN254_ERR_NOT_IN_SUBGROUP: return "G2 point not in the r-torsion subgroup";
    case BN254_ERR_INPUT_LEN: return "wrong number of public inputs"; case BN254_ERR_MALFORMED: return "malformed input";
    case BN254_ERR_OPENING_MISMATCH: return "opening polynomial mismatch"; case BN254_ERR_PAIRING_FAILED: return "pairing check failed";
    case BN254_ERR_BSB22_MISMATCH: return "BSB22 commitment count mismatch"; case BN254_ERR_INVERSE: return "inverse not found";
    default: return "unknown";
  }
}

// ---------------------------------------------------------------- gnark / SP1 formats (host only: byte shuffling and one square root)
int bn254_g1_compress(const uint8_t xy[64], uint8_t out[32]) {
  if (!xy || !out) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (!be_lt_p(xy) || !be_lt_p(xy + 32)) return set_err(BN254_E_BAD_ARG, "coordinate not reduced");
  G1Aff p; p.x = fp_from_be(xy); p.y = fp_from_be(xy + 32);
  enc_g1_compressed(out, p);
  return BN254_OK;
}
int bn254_g2_compress(const uint8_t xy[128], uint8_t out[64]) {
  if (!xy || !out) return set_err(BN254_E_BAD_ARG, "bad argument");
  for (int i = 0; i < 4; i++) if (!be_lt_p(xy + 32 * i)) return set_err(BN254_E_BAD_ARG, "coordinate not reduced");
  G2Aff p; p.x.c1 = fp_from_be(xy); p.x.c0 = fp_from_be(xy + 32); p.y.c1 = fp_from_be(xy + 64); p.y.c0 = fp_from_be(xy + 96);
  enc_g2_compressed(out, p);
  return BN254_OK;
}
int bn254_g1_decompress(const uint8_t in[32], uint8_t out[64], int checked, uint8_t* status) {
  if (!in || !out || !status) return set_err(BN254_E_BAD_ARG, "bad argument");
  G1Aff p;
  if (dec_g1_compressed(p, in) != DEC_OK) { *status = BN254_ERR_MALFORMED; return BN254_OK; }
  // checked (converter.rs:46-60): AffineG1::new = curve equation; G1 has cofactor 1, so there is nothing else to test
  if (checked && !g1_on_curve(p)) { *status = BN254_ERR_NOT_ON_CURVE; return BN254_OK; }
  enc_g1_uncompressed(out, p);
  *status = BN254_ACCEPT;
  return BN254_OK;
}
int bn254_g2_decompress(const uint8_t in[64], uint8_t out[128], unsigned mode, int checked, uint8_t* status) {
  if (!in || !out || !status || mode > 1) return set_err(BN254_E_BAD_ARG, "bad argument");
  G2Aff p;
  if (dec_g2_compressed(p, in, (int)mode) != DEC_OK) { *status = BN254_ERR_MALFORMED; return BN254_OK; }
  if (checked) {  // converter.rs:91-111: AffineG2::new = curve equation, then the r-torsion test
    if (!g2_on_curve(p)) { *status = BN254_ERR_NOT_ON_CURVE; return BN254_OK; }
    if (!g2_in_subgroup(p)) { *status = BN254_ERR_NOT_IN_SUBGROUP; return BN254_OK; }
  }
  enc_g2_uncompressed(out, p);
  *status = BN254_ACCEPT;
  return BN254_OK;
}
// SP1 v2.0.0 `SP1ProofWithPublicValues` as written by bincode (little-endian, u64 lengths): u32 variant (2 PlonK, 3 Groth16),
// String public_inputs[0], String public_inputs[1] (decimal), String encoded_proof (hex), String raw_proof (hex), [u8; 32]
// vkey hash, ...  (examples/script/src/main.rs:115-138 reads the same fields)
static bool sp1_string(const uint8_t* b, size_t len, size_t& off, const uint8_t** s, size_t* n) {
  if (off + 8 > len) return false;
  uint64_t k = 0; for (int i = 7; i >= 0; i--) k = k << 8 | b[off + i];
  off += 8;
  if (k > len - off) return false;
  *s = b + off; *n = (size_t)k; off += (size_t)k;
  return true;
}
static bool dec_to_be32(const uint8_t* s, size_t n, uint8_t out[32]) {
  memset(out, 0, 32);
  if (n == 0) return false;
  for (size_t i = 0; i < n; i++) {
    if (s[i] < '0' || s[i] > '9') return false;
    unsigned carry = s[i] - '0';
    for (int j = 31; j >= 0; j--) { unsigned v = out[j] * 10u + carry; out[j] = (uint8_t)v; carry = v >> 8; }
    if (carry) return false;  // more than 256 bits
  }
  return true;
}
int bn254_sp1_fixture_parse(const uint8_t* buf, size_t len, int* variant, uint8_t* raw_proof, size_t raw_cap, size_t* raw_len,
                            uint8_t public_inputs[64], uint8_t vkey_hash[32]) {
  if (!buf || !variant || !raw_proof || !raw_len || !public_inputs || !vkey_hash) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (len < 4) return set_err(BN254_E_BAD_ARG, "truncated fixture");
  *variant = (int)((uint32_t)buf[0] | (uint32_t)buf[1] << 8 | (uint32_t)buf[2] << 16 | (uint32_t)buf[3] << 24);
  size_t off = 4, n0, n1, ne, nr; const uint8_t *s0, *s1, *se, *sr;
  if (!sp1_string(buf, len, off, &s0, &n0) || !sp1_string(buf, len, off, &s1, &n1) || !sp1_string(buf, len, off, &se, &ne) ||
      !sp1_string(buf, len, off, &sr, &nr) || off + 32 > len)
    return set_err(BN254_E_BAD_ARG, "truncated fixture");
  if (!dec_to_be32(s0, n0, public_inputs) || !dec_to_be32(s1, n1, public_inputs + 32)) return set_err(BN254_E_BAD_ARG, "public input is not a decimal number below 2^256");
  if (nr % 2 || nr / 2 > raw_cap) return set_err(BN254_E_BAD_ARG, "raw proof does not fit");
  for (size_t i = 0; i < nr / 2; i++) {
    int v = 0;
    for (int k = 0; k < 2; k++) {
      uint8_t c = sr[2 * i + k];
      int d = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : (c >= 'A' && c <= 'F') ? c - 'A' + 10 : -1;
      if (d < 0) return set_err(BN254_E_BAD_ARG, "raw proof is not hexadecimal");
      v = v * 16 + d;
    }
    raw_proof[i] = (uint8_t)v;
  }
  *raw_len = nr / 2;
  memcpy(vkey_hash, buf + off, 32);
  return BN254_OK;
}

// The shard plan of a multi-device batch: the devices selected by device_mask in ascending order, shard k = the
// contiguous range [first[k], first[k] + count[k]) of the batch on devices[k]; balanced, the first n % w shards one proof longer (the same
// rule as sharding.shard_bounds of the multi-process job).  Host arithmetic only: needs no GPU, device_count is the caller's.
int bn254_shard_plan(size_t n, uint64_t device_mask, int device_count, int devices[64], size_t first[64], size_t count[64], int* n_shards) {
  if (!device_mask || !devices || !first || !count || !n_shards) return set_err(BN254_E_BAD_ARG, "bad argument");
  int w = 0;
  for (int b = 0; b < 64; b++)
    if ((device_mask >> b) & 1) {
      if (b >= device_count) return set_err(BN254_E_BAD_ARG, "device_mask selects a device that does not exist");
      devices[w++] = b;
    }
  const size_t base = n / (size_t)w, rem = n % (size_t)w;
  for (int r = 0; r < w; r++) { first[r] = (size_t)r * base + ((size_t)r < rem ? (size_t)r : rem); count[r] = base + ((size_t)r < rem ? 1 : 0); }
  *n_shards = w;
  return BN254_OK;
}

// ---- the gather of a multi-PROCESS job (one process per GPU): one ncclAllGather of the ranks' status bytes -----------------
// RCCL is not linked: a host that runs such a job already has it in its process (it created the communicator), so the symbol is looked up at the
// first call -- among the objects already loaded, then in librccl.so.
typedef int (*nccl_all_gather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static nccl_all_gather_fn rccl_all_gather() {
  static nccl_all_gather_fn fn = [] {
    void* sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
    if (!sym) { void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL); if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL); if (h) sym = dlsym(h, "ncclAllGather"); }
    return (nccl_all_gather_fn)sym;
  }();
  return fn;
}
int bn254_status_all_gather(void* nccl_comm, int world, int rank, const void* d_local, size_t n, void* d_full, void* d_scratch, void* hip_stream) {
  if (!nccl_comm || world <= 0 || world > 64 || rank < 0 || rank >= world || (n && (!d_local || !d_full))) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n == 0) return BN254_OK;
  int devs[64], nsh = 0; size_t first[64], cnt[64];
  int rc = bn254_shard_plan(n, world == 64 ? ~0ull : ((1ull << world) - 1), world, devs, first, cnt, &nsh);   // the ranks' contiguous ranges
  if (rc) return rc;
  nccl_all_gather_fn ag = rccl_all_gather();
  if (!ag) return set_err(BN254_E_HIP, "ncclAllGather not found: RCCL is neither loaded in this process nor loadable as librccl.so");
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t cap = (n + (size_t)world - 1) / (size_t)world;
  const int nccl_uint8 = 1;
  if (n % (size_t)world == 0) {
    // equal shards: the gathered blocks ARE the status vector
    int e = ag(d_local, d_full, cap, nccl_uint8, nccl_comm, s);
    return e ? set_err(BN254_E_HIP, "ncclAllGather failed (" + std::to_string(e) + ")") : BN254_OK;
  }
  // ragged: every rank sends a block of `cap` bytes (its shard, padded), in place in the scratch; the blocks are then packed into the vector
  if (!d_scratch) return set_err(BN254_E_BAD_ARG, "n is not a multiple of the world size: the gather needs world * ceil(n / world) bytes of scratch");
  uint8_t* sc = (uint8_t*)d_scratch;
  HIPCK(hipMemsetAsync(sc + (size_t)rank * cap, 0, cap, s));
  HIPCK(hipMemcpyAsync(sc + (size_t)rank * cap, d_local, cnt[rank], hipMemcpyDeviceToDevice, s));
  int e = ag(sc + (size_t)rank * cap, sc, cap, nccl_uint8, nccl_comm, s);
  if (e) return set_err(BN254_E_HIP, "ncclAllGather failed (" + std::to_string(e) + ")");
  for (int r = 0; r < world; r++)
    if (cnt[r]) HIPCK(hipMemcpyAsync((uint8_t*)d_full + first[r], sc + (size_t)r * cap, cnt[r], hipMemcpyDeviceToDevice, s));
  return BN254_OK;
}

}  // extern "C"

// The host half of the library is also built as ONE translation unit: tests/hostsan compiles this file with g++ against a stand-in HIP runtime (no hipcc,
// so no __HIPCC__) and drives the C ABI under the sanitizers.  There this file brings the other four files of the C ABI with it; hipcc builds each as its
// own object (Makefile).
#if !defined(__HIPCC__)
#include <array>
#include "bn254_capi_g16.hip"
#include "bn254_capi_plonk.hip"
#include "bn254_capi_sp1.hip"
#include "bn254_capi_dbg.hip"
#include "bn254_capi_selftest.hip"
// the device half of the self-test (bn254_selftest_dev.hip): nothing to launch in a host build, so every check "computes" its expected bytes and the device passes;
// tests/hostsan/hostsan_selftest.cpp brings a stand-in that can fail
#if !defined(BN254_HOSTSAN_SELFTEST)
int bn254_selftest_device(int, const std::vector<uint8_t>*, const bn254st::HostSide&, std::vector<uint8_t> got[bn254st::CK_COUNT], float gpu_ms[bn254st::MS_COUNT]) {
  for (int k = 0; k < bn254st::CK_COUNT; k++) got[k] = bn254_selftest_expected(k);
  for (int k = 0; k < bn254st::MS_COUNT; k++) gpu_ms[k] = 0.f;
  return BN254_OK;
}
#endif
// batches over many keys: tests/hostsan/hostsan_keys.cpp brings the file and stand-ins for its launchers; the older harness only needs the hook of bn254_groth16_vk_free
#if defined(BN254_HOSTSAN_KEYS)
#include "bn254_capi_keys.hip"
#else
void keys_sets_drop(const bn254_g16_pvk*) {}
// .. and, without the key-set file, nothing the loader probe over a key list could run on
int g16_keys_probe_loader(const bn254_g16_pvk* const*, size_t, const unsigned*, const uint8_t*, size_t, const uint8_t*, size_t, size_t, unsigned, int, size_t, unsigned*, uint8_t*, uint8_t*, size_t*,
                          int, void (*)(const uint8_t*, size_t, uint8_t*)) { return set_err(BN254_E_NO_DEVICE, "no key sets in this build"); }
#endif
// PlonK batches over many keys: tests/hostsan/hostsan_plonk_keys.cpp brings the file (after this one) and stand-ins for its launchers; every other harness only needs
// the hook of bn254_plonk_vk_free
#if !defined(BN254_HOSTSAN_PLONK_KEYS)
void plonk_keys_sets_drop(const bn254_plonk_pvk*) {}
// plonk_msm and the launch helpers of plonk_pass (bn254_capi_plonk.hip) name the launchers of a pass over a key list; without the key-set file nothing passes them one
hipError_t bn254_launch_g1_msm_rows_keys(const MsmPlan&, const int32_t*, const uint8_t*, size_t, int, int32_t*, int32_t*, const bn254::PlonkKeyDesc*, uint32_t, const uint32_t*, hipStream_t) {
  return hipErrorInvalidDeviceFunction;
}
hipError_t bn254_launch_plonk_stage1_keys(const bn254::PlonkKeyDesc*, uint32_t, const uint32_t*, const uint8_t*, size_t, size_t, const uint8_t*, size_t, size_t, size_t, const uint32_t*, void*, void*,
                                          uint8_t*, int, hipStream_t) { return hipErrorInvalidDeviceFunction; }
hipError_t bn254_launch_plonk_stage2_keys(const bn254::PlonkKeyDesc*, uint32_t, const uint32_t*, const uint8_t*, size_t, size_t, void*, const uint32_t*, const uint8_t*, void*, uint8_t*, uint8_t*,
                                          int, int, const uint32_t*, hipStream_t) { return hipErrorInvalidDeviceFunction; }
hipError_t bn254_launch_pairing2_fixed_keys(int32_t*, uint8_t*, size_t, const bn254::PlonkKeyDesc*, uint32_t, const uint32_t*, const int32_t*, int, hipStream_t) { return hipErrorInvalidDeviceFunction; }
#endif
// BN254_FLAG_RLC over a PlonK key list is honoured only from the threshold on (bn254_set_plonk_rlc_params), which tests/hostsan/hostsan_plonk_keys.cpp stays below: the
// joint check over keys is never reached there, and the harness that reaches it brings its own stand-in (tests/hostsan/hostsan_plonk_keys_rlc.cpp)
#if !defined(BN254_HOSTSAN_PLONK_KEYS_RLC)
hipError_t bn254_launch_pairing2_fixed_groups_keys(int32_t*, uint8_t*, size_t, const bn254::PlonkKeyDesc*, uint32_t, const uint32_t*, const int32_t*, int, hipStream_t) {
  return hipErrorInvalidDeviceFunction;
}
#endif
// the direct form of a batch over many keys: a host build starts with the knob at 0 (bn254_capi_keys.hip), so this is never reached unless a harness turns the knob --
// and that harness brings its own stand-in (tests/hostsan/hostsan_keys_small.cpp)
#if defined(BN254_HOSTSAN_KEYS) && !defined(BN254_HOSTSAN_KEYS_DIRECT)
hipError_t bn254_launch_g16_keys_direct(const G16KeysDirectArgs&, hipStream_t) { return hipErrorInvalidDeviceFunction; }
#endif
#if defined(BN254_HOSTSAN_KEYS)
hipError_t bn254_coop12_prepare() { return hipSuccess; }      // the step-kind table of the cooperative kernels: nothing to create without a device compiler
void bn254_launch_g16_prepare_keys(const G16KeysLaunchArgs&, unsigned, hipStream_t) {}      // the loader probe over a key list (g16_keys_probe_loader): no kernels in a host build
#endif
// the launchers of the value-level probes (bn254_capi_dbg.hip: bn254_dbg_coop12_op, bn254_dbg_verdict, ..): no kernels in a host build, so the probes there check
// their arguments, move their buffers and return what those held; every harness links these, whichever stand-ins it brings for the launchers of the product
hipError_t bn254_launch_dbg_fp12_op_fmt(int, const uint8_t*, const uint8_t*, uint8_t*, size_t, int32_t*, uint8_t*, int, int, hipStream_t) { return hipSuccess; }
hipError_t bn254_launch_dbg_load(int32_t*, size_t, uint8_t*, int, const void*, int, hipStream_t) { return hipSuccess; }
hipError_t bn254_launch_dbg_store(int32_t*, size_t, int, void*, int, hipStream_t) { return hipSuccess; }
hipError_t bn254_launch_dbg_verdict(int, int32_t*, size_t, uint8_t*, const int32_t*, hipStream_t) { return hipSuccess; }
hipError_t bn254_launch_dbg_coop12_g16(const G16LaunchArgs&, hipStream_t) { return hipSuccess; }
void bn254_launch_g16_loader(const G16LaunchArgs&, const G16LoaderForm&, hipStream_t, G16Prof*, G16LoaderRan*) {}
hipError_t bn254_coop12_dbg_op(int32_t*, uint8_t*, size_t, int, int, const int32_t*, hipStream_t) { return hipSuccess; }
hipError_t bn254_coop12_miller_fixed_keys(int32_t*, uint8_t*, size_t, const uint32_t*, uint32_t, const bn254::PlonkKeyDesc*, uint32_t, const int32_t*, int, hipStream_t) { return hipSuccess; }
hipError_t bn254_coop12_miller_fixed(int32_t*, uint8_t*, size_t, int, const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) { return hipSuccess; }
// Without a device compiler there is no k_g16_decompress / k_g16_status_merge: the host build runs their bodies (bn254_codec.h) in place, synchronously, on
// the host memory such a build allocates.  hipcc builds never see these definitions; the library's launchers are in bn254_k_g16_load.hip.
hipError_t bn254_launch_g16_decompress(const uint8_t* src, size_t stride, uint32_t n, uint8_t* raw, uint8_t* pre, hipStream_t) {
  // (the harness's batches of 2^20 proofs repeat a few records: results are kept by record, three square roots per record are not made again)
  struct Memo { uint32_t out[64]; uint8_t pre; };
  thread_local std::map<std::array<uint32_t, 32>, Memo> memo;
  for (uint32_t i = 0; i < n; i++) {
    std::array<uint32_t, 32> in;
    memcpy(in.data(), src + (size_t)i * stride, 128);
    auto it = memo.find(in);
    if (it == memo.end()) {
      if (memo.size() >= 4096) memo.clear();
      Memo m;
      m.pre = g16_decompress_record(in.data(), m.out) ? 0 : 1;
      it = memo.emplace(in, m).first;
    }
    pre[i] = it->second.pre;
    memcpy(raw + (size_t)i * 256, it->second.out, 256);
  }
  return hipSuccess;
}
hipError_t bn254_launch_g16_status_merge(uint8_t* status, const uint8_t* pre, uint32_t n, hipStream_t) {
  for (uint32_t i = 0; i < n; i++) if (pre[i]) status[i] = BN254_ST_MALFORMED;
  return hipSuccess;
}
hipError_t bn254_launch_sp1_public_inputs(const uint8_t* vkh, size_t vkh_stride, const uint8_t* pv, uint64_t pv_bytes, uint64_t pv_base, const uint64_t* off, uint32_t n,
                                          uint8_t* rows, uint8_t* pre, hipStream_t) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t row[16];
    pre[i] = bn254::sp1_row(vkh + (size_t)i * vkh_stride, pv, pv_bytes, pv_base, off[i], off[i + 1], row) ? 0 : 1;
    memcpy(rows + (size_t)i * 64, row, 64);
  }
  return hipSuccess;
}
#endif
