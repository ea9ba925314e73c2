// bn254_capi_sp1.hip -- the SP1 entries of the C ABI (include/bn254_verify.h, "SP1 proofs from their public values"): a proof comes with its program's vkey hash
// and public values, and the two circuit inputs vkey_hash | SHA-256(values) & mask are made on the device (k_sp1_public_inputs, bn254_sha256.h) before the
// unchanged Groth16 or PlonK pipeline runs with n_public = 2.  Also the host digest and the test probe of the kernel body.
#include "bn254_capi_internal.h"
#include "bn254_kernels.h"
#include "bn254_sha256.h"

using namespace bn254;

// The argument check of every SP1 batch entry, made before any device is touched: everything check_batch_args checks for a raw batch with n_public = 2, plus the
// vkey hashes (stride 0 or >= 32), the offsets and the values.  host_offsets: the offsets are host memory and are checked to be non-decreasing here (the device
// entries cannot read them: a bad range there is the proof's MALFORMED status).
int check_sp1_args(bool plonk, const void* pvk, const void* proofs, size_t proof_stride, const void* vkh, size_t vkh_stride, const void* pv, uint64_t pv_bytes,
                   const uint64_t* off, bool host_offsets, size_t n, const void* status, unsigned flags) {
  if (vkh_stride && vkh_stride < 32) return set_err(BN254_E_BAD_ARG, "vkey_stride must be 0 (one vkey hash for the batch) or at least 32");
  if (plonk && (flags & ~(unsigned)BN254_FLAG_RLC)) return set_err(BN254_E_BAD_ARG, "unknown flag (the SP1 PlonK entries know BN254_FLAG_RLC)");
  int rc = check_batch_args(plonk, pvk, proofs, proof_stride, vkh, 2, n, status, flags);
  if (rc || n == 0) return rc;
  if (!vkh || !off) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > SIZE_MAX / 64 - 1 || (vkh_stride && vkh_stride > SIZE_MAX / n)) return set_err(BN254_E_BAD_ARG, "n too large");
  if (host_offsets) {
    for (size_t i = 0; i < n; i++)
      if (off[i + 1] < off[i]) return set_err(BN254_E_BAD_ARG, "pv_offsets decrease at proof " + std::to_string(i));
    pv_bytes = off[n] - off[0];
  }
  if (pv_bytes && !pv) return set_err(BN254_E_BAD_ARG, "bad argument");
  return BN254_OK;
}

namespace {
// A buffer of PlonkDev::sp1_bufs held by one SP1 PlonK call: the smallest free one that is large enough, else a new one (a free buffer that is too small is
// replaced, the only hipFree on this path).  Returned to the device's list when the call ends; every path out of a call has drained the work that used it.
struct Sp1PlonkBuf {
  PlonkDev* d; DevBuf<uint8_t> p;
  explicit Sp1PlonkBuf(PlonkDev* d_) : d(d_) {}
  int take(size_t need) {
    std::lock_guard<std::mutex> lk(d->sp1_mu);
    auto& v = d->sp1_bufs;
    int best = -1, largest = 0;
    for (int i = 0; i < (int)v.size(); i++) {
      if (v[i].cap() >= need && (best < 0 || v[i].cap() < v[best].cap())) best = i;
      if (v[i].cap() > v[largest].cap()) largest = i;
    }
    if (best >= 0) { p = std::move(v[best]); v.erase(v.begin() + best); return BN254_OK; }
    if (!v.empty()) v.erase(v.begin() + largest);   // none is large enough: the largest gives way
    return p.ensure((need + ((size_t)1 << 20) - 1) >> 20 << 20);
  }
  ~Sp1PlonkBuf() {
    if (!p) return;
    std::lock_guard<std::mutex> lk(d->sp1_mu);
    d->sp1_bufs.push_back(std::move(p));
  }
};
int sp1_plonk_dev(const bn254_plonk_pvk* pvk, int device, PlonkDev** d) {
  std::lock_guard<std::mutex> lk(pvk->mu);
  return plonk_ensure_dev(pvk, device, d);
}
// the rows of n proofs on `s` in launches of at most G16_MAX_BATCH proofs (pre: n bytes)
int sp1_rows_enqueue(const Sp1Src& src, size_t n, uint8_t* rows, uint8_t* pre, hipStream_t s) {
  for (size_t o = 0; o < n; o += G16_MAX_BATCH) {
    const size_t m = n - o < (size_t)G16_MAX_BATCH ? n - o : (size_t)G16_MAX_BATCH;
    hipError_t e = bn254_launch_sp1_public_inputs(src.vkh + o * src.vkh_stride, src.vkh_stride, src.pv, src.pv_bytes, src.pv_base, src.off + o, (uint32_t)m,
                                                  rows + o * 64, pre + o, s);
    if (e != hipSuccess) return launch_err(e, "SP1 public inputs");
  }
  return BN254_OK;
}
// a call's copy of host vkey hashes, values and offsets in device memory: vkey hashes compacted to 32 bytes per proof (or the one hash of stride 0), the values
// [off[0], off[n]) of the caller's buffer (so pv_base = off[0]), the offsets as they are
size_t sp1_stage_bytes(size_t vkh_stride, const uint64_t* off, size_t n) { return (n + 1) * 8 + (vkh_stride ? n * 32 : 32) + (off[n] - off[0]); }
int sp1_stage_host(const uint8_t* vkh, size_t vkh_stride, const uint8_t* pv, const uint64_t* off, size_t n, uint8_t* dst, Sp1Src* out, hipStream_t s) {
  const size_t vk_bytes = vkh_stride ? n * 32 : 32, pv_total = off[n] - off[0], off_bytes = (n + 1) * 8;
  uint8_t* d_off = dst; uint8_t* d_vk = dst + off_bytes; uint8_t* d_pv = d_vk + vk_bytes;
  HIPCK(hipMemcpyAsync(d_off, off, off_bytes, hipMemcpyHostToDevice, s));
  if (vkh_stride == 0 || vkh_stride == 32) HIPCK(hipMemcpyAsync(d_vk, vkh, vk_bytes, hipMemcpyHostToDevice, s));
  else {
    std::vector<uint8_t> packed(vk_bytes);
    for (size_t i = 0; i < n; i++) memcpy(packed.data() + 32 * i, vkh + i * vkh_stride, 32);
    HIPCK(hipMemcpyAsync(d_vk, packed.data(), vk_bytes, hipMemcpyHostToDevice, s));
    HIPCK(hipStreamSynchronize(s));   // `packed` is about to go
  }
  if (pv_total) HIPCK(hipMemcpyAsync(d_pv, pv + off[0], pv_total, hipMemcpyHostToDevice, s));
  *out = Sp1Src{d_vk, (size_t)(vkh_stride ? 32 : 0), d_pv, pv_total, off[0], (const uint64_t*)d_off};
  return BN254_OK;
}
}  // namespace

extern "C" {

int bn254_sp1_public_values_digest(const uint8_t* public_values, size_t len, uint8_t out[32]) {
  if (!out || (len && !public_values)) return set_err(BN254_E_BAD_ARG, "bad argument");
  uint32_t w[8];
  sp1_digest(public_values, len, 0, len, w);
  memcpy(out, w, 32);
  return BN254_OK;
}

int bn254_sp1_groth16_verify_batch(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* vkey_hashes, size_t vkey_stride,
                                   const uint8_t* public_values, const uint64_t* pv_offsets, size_t n, uint8_t* status, int device, unsigned flags) {
  int rc = check_sp1_args(false, pvk, proofs, proof_stride, vkey_hashes, vkey_stride, public_values, 0, pv_offsets, true, n, status, flags);
  if (rc || n == 0) return rc;
  return g16_sp1_host(pvk, proofs, proof_stride, Sp1Src{vkey_hashes, vkey_stride, public_values, 0, 0, pv_offsets}, n, status, device, flags);
}

int bn254_sp1_groth16_verify_batch_device(const bn254_g16_pvk* pvk, const void* d_proofs, size_t proof_stride, const void* d_vkey_hashes, size_t vkey_stride,
                                          const void* d_public_values, size_t pv_bytes, const uint64_t* d_pv_offsets, size_t n, void* d_status, int device,
                                          void* hip_stream, unsigned flags) {
  int rc = check_sp1_args(false, pvk, d_proofs, proof_stride, d_vkey_hashes, vkey_stride, d_public_values, pv_bytes, d_pv_offsets, false, n, d_status, flags);
  if (rc || n == 0) return rc;
  const Sp1Src s{(const uint8_t*)d_vkey_hashes, vkey_stride, (const uint8_t*)d_public_values, pv_bytes, 0, d_pv_offsets};
  return g16_sp1_device(pvk, d_proofs, proof_stride, s, n, d_status, device, (hipStream_t)hip_stream, flags);
}

// PlonK: calls on one key run side by side on the key's contexts (PlonkLease), so the rows of a call live in a buffer that call holds (Sp1PlonkBuf), never in
// the key's state.
int bn254_sp1_plonk_verify_batch(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* vkey_hashes, size_t vkey_stride,
                                 const uint8_t* public_values, const uint64_t* pv_offsets, size_t n, uint8_t* status, int device, unsigned flags) {
  int rc = check_sp1_args(true, pvk, proofs, proof_stride, vkey_hashes, vkey_stride, public_values, 0, pv_offsets, true, n, status, flags);
  if (rc || n == 0) return rc;
  PlonkDev* d;
  if ((rc = sp1_plonk_dev(pvk, device, &d))) return rc;
  const hipStream_t s = nullptr;   // the null stream: the context streams of the passes are non-blocking, so it does not wait for other calls' work
  Sp1PlonkBuf buf(d);
  const size_t row_bytes = (n * 65 + 255) / 256 * 256;   // the staged offsets after the rows and pre bytes, 8-byte aligned
  if ((rc = buf.take(row_bytes + sp1_stage_bytes(vkey_stride, pv_offsets, n)))) return rc;
  uint8_t* rows = buf.p;
  Sp1Src src;
  if ((rc = sp1_stage_host(vkey_hashes, vkey_stride, public_values, pv_offsets, n, rows + row_bytes, &src, s)) || (rc = sp1_rows_enqueue(src, n, rows, rows + n * 64, s))) {
    const std::string keep = g_err;
    (void)hipStreamSynchronize(s);
    g_err = keep;
    return rc;
  }
  HIPCK(hipStreamSynchronize(s));
  // the offsets were checked on the host: every range is inside the staged values and no pre byte is set
  return plonk_batch_rows(pvk, proofs, proof_stride, rows, n, status, device, flags, false);
}

int bn254_sp1_plonk_verify_batch_device(const bn254_plonk_pvk* pvk, const void* d_proofs, size_t proof_stride, const void* d_vkey_hashes, size_t vkey_stride,
                                        const void* d_public_values, size_t pv_bytes, const uint64_t* d_pv_offsets, size_t n, void* d_status, int device,
                                        void* hip_stream, unsigned flags) {
  int rc = check_sp1_args(true, pvk, d_proofs, proof_stride, d_vkey_hashes, vkey_stride, d_public_values, pv_bytes, d_pv_offsets, false, n, d_status, flags);
  if (rc || n == 0) return rc;
  PlonkDev* d;
  if ((rc = sp1_plonk_dev(pvk, device, &d))) return rc;
  const hipStream_t s = (hipStream_t)hip_stream;
  Sp1PlonkBuf buf(d);
  if ((rc = buf.take(n * 65))) return rc;
  const Sp1Src src{(const uint8_t*)d_vkey_hashes, vkey_stride, (const uint8_t*)d_public_values, pv_bytes, 0, d_pv_offsets};
  uint8_t* rows = buf.p;
  uint8_t* pre = rows + n * 64;
  if ((rc = sp1_rows_enqueue(src, n, rows, pre, s))) { const std::string keep = g_err; (void)hipStreamSynchronize(s); g_err = keep; return rc; }
  HIPCK(hipStreamSynchronize(s));   // also what the caller's stream still had to do to the inputs: the passes run on the key's own context streams
  if ((rc = plonk_batch_rows(pvk, (const uint8_t*)d_proofs, proof_stride, rows, n, (uint8_t*)d_status, device, flags, true))) return rc;
  for (size_t o = 0; o < n; o += G16_MAX_BATCH) {
    const size_t m = n - o < (size_t)G16_MAX_BATCH ? n - o : (size_t)G16_MAX_BATCH;
    hipError_t e = bn254_launch_g16_status_merge((uint8_t*)d_status + o, pre + o, (uint32_t)m, s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return set_err(BN254_E_HIP, std::string("kernel launch (status merge): ") + hipGetErrorString(e)); }
  }
  HIPCK(hipStreamSynchronize(s));
  return BN254_OK;
}

int bn254_dbg_g16_sp1_alloc(size_t n, uint64_t out[3]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  const G16Sp1Alloc a = g16_sp1_alloc(n);
  out[0] = a.proofs; out[1] = a.row_bytes; out[2] = a.pre_bytes;
  return BN254_OK;
}

// the body of k_sp1_public_inputs: device -1 runs it compiled for the host (bn254_sha256.h::sp1_row), device >= 0 launches the kernel on copies of the buffers
int bn254_dbg_sp1_public_inputs(const uint8_t* vkey_hashes, size_t vkey_stride, const uint8_t* public_values, size_t pv_bytes, const uint64_t* pv_offsets, size_t n,
                                uint8_t* rows_out, uint8_t* bad_out, int device) {
  if ((n && (!vkey_hashes || !pv_offsets || !rows_out || !bad_out)) || (vkey_stride && vkey_stride < 32) || (pv_bytes && !public_values) || device < -1 ||
      n > SIZE_MAX / 64 - 1 || (n && vkey_stride > SIZE_MAX / n))
    return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n == 0) return BN254_OK;
  if (device < 0) {
    for (size_t i = 0; i < n; i++) {
      uint32_t row[16];
      bad_out[i] = sp1_row(vkey_hashes + i * vkey_stride, public_values, pv_bytes, 0, pv_offsets[i], pv_offsets[i + 1], row) ? 0 : 1;
      memcpy(rows_out + 64 * i, row, 64);
    }
    return BN254_OK;
  }
  int rc = check_device(device);
  if (rc) return rc;
  const size_t vk_bytes = vkey_stride ? (n - 1) * vkey_stride + 32 : 32, off_bytes = (n + 1) * 8;
  DevBuf<uint8_t> b;
  if ((rc = b.ensure(off_bytes + n * 65 + vk_bytes + (pv_bytes ? pv_bytes : 4)))) return rc;
  uint8_t *d_off = b, *d_rows = b + off_bytes, *d_pre = d_rows + n * 64, *d_vk = d_pre + n, *d_pv = d_vk + vk_bytes;
  HIPCK(hipMemcpy(d_off, pv_offsets, off_bytes, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(d_vk, vkey_hashes, vk_bytes, hipMemcpyHostToDevice));
  if (pv_bytes) HIPCK(hipMemcpy(d_pv, public_values, pv_bytes, hipMemcpyHostToDevice));
  const Sp1Src src{d_vk, vkey_stride, d_pv, pv_bytes, 0, (const uint64_t*)d_off};
  if ((rc = sp1_rows_enqueue(src, n, d_rows, d_pre, nullptr))) return rc;
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(rows_out, d_rows, n * 64, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(bad_out, d_pre, n, hipMemcpyDeviceToHost));
  return BN254_OK;
}

}  // extern "C"
