// bn254_k_keys.hip -- the kernels of a Groth16 batch over many verifying keys (bn254_keys.h; bn254_groth16_verify_batch_keys): the proofs are brought into slots so
// that every wavefront works for one key, and the four places where a key enters the single-key pipeline read it from the wavefront's descriptor instead of the
// launch arguments.  Everything in between (the final exponentiation program up to its last product) never sees a key and runs unchanged on the slots.
//   k_keys_count / k_keys_scan / k_keys_place   per-key histogram of key_index, exclusive scan of the counts rounded up to a granule, slot -> proof and granule -> key
//   k_g16_prepare_keys      k_g16_prepare through the slot index: record and input row of the slot's proof, L from the key's byte-window tables
//   k_g16_check_scalars_keys  BN254_FLAG_STRICT_SCALARS with the key's input count
//   k_f12_mul_verdict_keys  the last product of the final exponentiation, the comparison with the key's e(alpha, beta) and the scatter of every slot's status byte
//                           back to proof order
// (k_miller_run_keys is in bn254_k_miller.hip, beside the kernel it is an instance of: its first launch sets f and T, its last one tests B's subgroup with the key's
// inputs_match.)
#include <hip/hip_runtime.h>
#include "bn254_devws.h"
#include "bn254_g16_loader.h"
#include "bn254_keys.h"

namespace bn254 {

// ---- grouping ---------------------------------------------------------------------------------------------------------------------------------------------
#define KEYS_LDS_COUNTERS 8192   // key lists up to this long are counted in LDS (32 KB) and flushed once per workgroup
__global__ void __launch_bounds__(256) k_keys_count(const uint32_t* __restrict__ key_index, uint32_t n, uint32_t n_keys, uint32_t* __restrict__ count) {
  __shared__ uint32_t lc[KEYS_LDS_COUNTERS];
  const bool priv = n_keys <= KEYS_LDS_COUNTERS;
  if (priv) { for (uint32_t k = threadIdx.x; k < n_keys; k += 256) lc[k] = 0; __syncthreads(); }
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t k = key_index[i];
    if (k >= n_keys) continue;
    if (priv) atomicAdd(&lc[k], 1u); else atomicAdd(&count[k], 1u);
  }
  if (priv) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n_keys; k += 256) { const uint32_t c = lc[k]; if (c) atomicAdd(&count[k], c); }
  }
}
// one workgroup of 1024 lanes: lane t scans keys [t per, (t + 1) per), the lanes' totals are scanned through LDS.  base[k]: first slot of key k; cursor[k]: the same,
// advanced by k_keys_place; n_slots[0]: slots of the batch
__global__ void __launch_bounds__(1024) k_keys_scan(const uint32_t* __restrict__ count, uint32_t n_keys, uint32_t* __restrict__ base, uint32_t* __restrict__ cursor, uint32_t* __restrict__ n_slots) {
  __shared__ uint32_t tot[1024];
  const uint32_t t = threadIdx.x, per = (n_keys + 1023u) / 1024u;
  const uint32_t lo = t * per < n_keys ? t * per : n_keys, hi = lo + per < n_keys ? lo + per : n_keys;
  uint32_t mine = 0;
  for (uint32_t k = lo; k < hi; k++) mine += keys_round_up(count[k]);
  tot[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {   // inclusive scan of the lanes' totals
    const uint32_t v = t >= d ? tot[t - d] : 0u;
    __syncthreads();
    tot[t] += v;
    __syncthreads();
  }
  const uint32_t after = keys_scan_range(count, base, lo, hi, tot[t] - mine);
  for (uint32_t k = lo; k < hi; k++) cursor[k] = base[k];
  (void)after;
  if (t == 1023) n_slots[0] = tot[1023];
}
// proof i takes the next slot of its key.  The lanes of a wavefront that hold the same key take their slots with ONE atomic (a batch of one key would otherwise send
// every proof to the same counter); an index outside the list gets no slot and the proof's status is MALFORMED.
__global__ void __launch_bounds__(256) k_keys_place(const uint32_t* __restrict__ key_index, uint32_t n, uint32_t n_keys, uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ slot_to_proof, uint32_t* __restrict__ granule_key, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t k = i < n ? key_index[i] : 0xffffffffu;
  bool todo = i < n && k < n_keys;
  if (i < n && k >= n_keys) status[i] = BN254_ST_MALFORMED;
  const uint32_t lane = threadIdx.x & 63u;
  for (;;) {
    const uint64_t left = __builtin_amdgcn_ballot_w64(todo);
    if (left == 0) break;
    const uint32_t lead = (uint32_t)__builtin_ctzll(left);
    const uint32_t kk = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)lead);
    const uint64_t same = __builtin_amdgcn_ballot_w64(todo && k == kk);
    uint32_t first = 0;
    if (lane == lead) first = atomicAdd(&cursor[kk], (uint32_t)__builtin_popcountll(same));
    first = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)lead);
    if (todo && k == kk) {
      keys_place(slot_to_proof, granule_key, first + (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull)), i, k);
      todo = false;
    }
  }
}

// ---- k_g16_prepare_keys ---------------------------------------------------------------------------------------------------------------------------------------
// The launch covers slots [0, m) of ws / slot_status; slot_to_proof and granule_key point at the launch's first slot / granule.  live_slots: slots of the launch that
// exist (n_slots[0] - slot0, clamped to m); every other slot, padding slots and slots whose proof index is out of range get status 0: not pending, so no later
// kernel works on them.  The staging of the records and the parse of A, B, C are k_g16_prepare's (bn254_g16_loader.h).
__global__ void __launch_bounds__(256, 2)
k_g16_prepare_keys(const uint8_t* __restrict__ proofs, size_t stride, const uint8_t* __restrict__ inputs, size_t input_stride, uint32_t n_proofs, uint32_t m, uint32_t slot0,
                   const uint32_t* __restrict__ n_slots, const uint32_t* __restrict__ slot_to_proof, const uint32_t* __restrict__ granule_key,
                   const G16KeyDesc* __restrict__ desc, uint32_t n_keys, int32_t* ws, uint8_t* __restrict__ slot_status) {
  __shared__ uint32_t lds[4 * 64 * PREP_LDS_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t first = blockIdx.x * 256u + (uint32_t)wave * 64u;
  const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_slots[0]);
  const uint32_t live_slots = total > slot0 ? (total - slot0 < m ? total - slot0 : m) : 0u;
  const bool wave_live = first < live_slots;       // granules are whole: a live wavefront's 64 slots all exist
  const uint32_t i = first + lane;
  uint32_t pi = wave_live ? slot_to_proof[i] : G16_KEYS_NO_PROOF;
  const bool live = pi < n_proofs;
  uint32_t* wl = lds + wave * 64 * PREP_LDS_ROW;
  if (wave_live) g16_stage_records(wl, proofs, stride, n_proofs, lane, pi);      // the record of slot j of this wave: its index from lane j
  __syncthreads();
  if (!wave_live) { if (i < m) slot_status[i] = 0; return; }
  const KeyView kv = keys_view(desc, granule_key, first, n_keys);
  // padding lanes get an out-of-range lane offset: the descriptor's bounds check drops their stores
  DevWs w(ws, m, live ? i : DEAD_LANE);
  const uint32_t* my = wl + lane * PREP_LDS_ROW;

  // ---- A, then B: the first error in the reference's order -- A, then B (member, curve), B subgroup (the tail of k_miller_run_keys), then C
  G1Aff A;
  int err = g16_parse_a(my, A);
  w.st(VE_AX, A.x); w.st(VE_AY, A.y);
  G2Aff B;
  err = g16_parse_b(my, B, err);
  vst2(w, VE_B, B.x); vst2(w, VE_B + 2, B.y);
  G1Aff C;
  const int err_c = g16_parse_c(my, C);
  w.st(VE_CX, C.x); w.st(VE_CY, C.y);

  // ---- L = K0 + sum_s x_s K_s over the KEY's inputs (the loop bound is wavefront-uniform), x_s taken as raw 256-bit integers; byte windows: 32 table additions per
  // input (the set's tables are 0.65 MB per point where a key's own 13-bit windows are 13 MB: bn254_capi_keys.hip)
  const int32_t* k0 = kv.k0;
  const int32_t* msm_tab = kv.msm_tab;
  const int n_public = kv.inputs_match ? kv.n_public : 0;
  G1Aff K0; K0.x = uni_ld(k0); K0.y = uni_ld(k0 + BN_NL);
  G1Proj L = g1_from_affine(K0);
  for (int s = 0; s < n_public; s++) {
    uint32_t sw[8];
#pragma unroll
    for (int k = 0; k < 8; k++) sw[k] = 0u;       // a padding lane adds nothing
    if (live) {
      const uint8_t* sp = inputs + (size_t)pi * input_stride + (size_t)s * 32;
      if (((((uintptr_t)inputs) | input_stride) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) sw[k] = ((const uint32_t*)sp)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) sw[k] = (uint32_t)sp[4 * k] | (uint32_t)sp[4 * k + 1] << 8 | (uint32_t)sp[4 * k + 2] << 16 | (uint32_t)sp[4 * k + 3] << 24;
      }
    }
    for (int j = 0; j < 32; j++) {  // byte j of the big-endian scalar = window 31 - j (as in k_g16_msm_partial)
      const int wi = 31 - j;
      const uint32_t dig = sw[0] & 0xff;
#pragma unroll
      for (int k = 0; k < 7; k++) sw[k] = (sw[k] >> 8) | (sw[k + 1] << 24);
      sw[7] >>= 8;
      if (dig != 0) L = g1_add_mixed(L, msm_entry(msm_tab, (size_t)(s * 32 + wi) * 255 + (dig - 1)));
    }
  }
  bool l_inf = g1_is_identity(L);
  G1Aff La = g1_to_affine(L);
  La.y = fp_select(l_inf, fp_one(), La.y);
  w.st(VE_LX, La.x); w.st(VE_LY, La.y);
  slot_status[i] = !live ? (uint8_t)0 : err ? (uint8_t)err : (uint8_t)(BN254_ST_PENDING | (l_inf ? BN254_ST_LINF : 0) | err_c);
}

// BN254_FLAG_STRICT_SCALARS (k_g16_check_scalars): a public input >= r makes the proof NOT_MEMBER ahead of every other outcome; the inputs counted are the key's
__global__ void __launch_bounds__(256, 2)
k_g16_check_scalars_keys(const uint8_t* __restrict__ inputs, size_t input_stride, uint32_t n_proofs, uint32_t m, const uint32_t* __restrict__ slot_to_proof,
                         const uint32_t* __restrict__ granule_key, const G16KeyDesc* __restrict__ desc, uint32_t n_keys, uint8_t* __restrict__ slot_status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t first = i & ~63u;
  if (first >= m) return;
  // status 0 is what k_g16_prepare_keys leaves in every slot without a proof (no loader status is 0): such a wavefront has no descriptor to read
  const uint8_t st = slot_status[i];
  if (__builtin_amdgcn_ballot_w64(st != 0) == 0) return;
  const int n_public = keys_view(desc, granule_key, first, n_keys).n_public;
  const uint32_t pi = slot_to_proof[i];
  if (st == 0 || pi >= n_proofs) return;
  bool bad = false;
  for (int s = 0; s < n_public; s++) {
    uint32_t w[8];
    words_from_be(w, inputs + (size_t)pi * input_stride + (size_t)s * 32);
    bad |= words_ge(w, BN_R_WORDS);
  }
  if (bad) slot_status[i] = BN254_ST_NOT_MEMBER;
}

// the last product of the final exponentiation, compared with e(alpha, beta) of the wavefront's key as it is stored (bn254_vm.h::vm_f12_mul_eq_const); then every slot
// that holds a proof hands its status byte -- the verdict, or what an earlier kernel decided -- to the proof, also in a wavefront none of whose proofs is pending
__global__ void __launch_bounds__(256, 2)
k_f12_mul_verdict_keys(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, const uint32_t* __restrict__ slot_to_proof, const uint32_t* __restrict__ granule_key,
                       const G16KeyDesc* __restrict__ desc, uint32_t n_keys, uint32_t n_proofs, uint8_t* __restrict__ out_status, int e_dst, int e_a, int e_b) {
  __shared__ int32_t park_lds[72 * 256];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if ((i & ~63u) >= n) return;
  const uint8_t st = status[i < n ? i : n - 1];
  if (__builtin_amdgcn_ballot_w64(st != 0) == 0) return;      // no proof in this wavefront's slots
  uint8_t out = st;
  if (__builtin_amdgcn_ballot_w64((st & BN254_ST_PENDING) != 0) != 0) {
    DevWs w(ws, n, i < n ? i : DEAD_LANE);
    w.lds = park_lds;
    const int32_t* target = keys_view(desc, granule_key, i & ~63u, n_keys).target;
    const bool acc = vm_f12_mul_eq_const(w, e_dst, e_a, e_b, target);
    if (st & BN254_ST_PENDING) out = acc ? BN254_ST_ACCEPT : BN254_ST_REJECT;
  }
  if (i < n && st != 0) { const uint32_t pi = slot_to_proof[i]; if (pi < n_proofs) out_status[pi] = out; }
}

// ---- PlonK batches over many keys: the records and input rows of a pass into slot order, the slots' status bytes back ------------------------------------------
// One wavefront per slot, the lanes on consecutive dwords (a byte path for unaligned sources, as k_gather_rows).  Of a proof's input row only the 32 n_public(key)
// bytes of its key are read; the rest of the slot's row, and the whole record and row of a padding slot, are zero -- an all-zero record is malformed for every key
// (its count of claimed values is not 6 + n_qcp), so stage 1 decides a padding slot and nothing later sees it as pending.
__global__ void __launch_bounds__(256) k_plonk_keys_gather(const uint8_t* __restrict__ proofs, size_t stride, const uint8_t* __restrict__ inputs, size_t input_stride, uint32_t n_proofs,
                                                           const uint32_t* __restrict__ slot_to_proof, const uint32_t* __restrict__ granule_key, const PlonkKeyDesc* __restrict__ desc,
                                                           uint32_t n_keys, uint32_t m, uint8_t* __restrict__ recs, uint32_t rec_stride, uint32_t rec_bytes, uint8_t* __restrict__ rows,
                                                           uint32_t row_stride) {
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (j >= m) return;
  const uint32_t pi = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot_to_proof[j]);
  const bool live = pi < n_proofs;
  uint32_t* dr = (uint32_t*)(recs + (size_t)j * rec_stride);
  const uint8_t* sr = proofs + (size_t)(live ? pi : 0) * stride;
  const bool aligned = ((((uintptr_t)proofs) | stride) & 3) == 0;
  for (uint32_t d = lane; d < rec_stride / 4; d += 64) {
    uint32_t v = 0;
    if (live && 4 * d < rec_bytes) {
      if (aligned) v = *(const uint32_t*)(sr + 4 * (size_t)d);
      else { const uint8_t* p = sr + 4 * (size_t)d; for (uint32_t b = 0; b < 4 && 4 * d + b < rec_bytes; b++) v |= (uint32_t)p[b] << (8 * b); }   // (never past the last record)
    }
    dr[d] = v;
  }
  if (row_stride == 0) return;
  const uint32_t in_bytes = live ? 32u * plonk_keys_view(desc, granule_key, j & ~63u, n_keys).n_public : 0u;
  uint32_t* di = (uint32_t*)(rows + (size_t)j * row_stride);
  const uint8_t* si = inputs + (size_t)(live ? pi : 0) * input_stride;
  const bool in_aligned = ((((uintptr_t)inputs) | input_stride) & 3) == 0;
  for (uint32_t d = lane; d < row_stride / 4; d += 64) {
    uint32_t v = 0;
    if (4 * d < in_bytes) {
      if (in_aligned) v = *(const uint32_t*)(si + 4 * (size_t)d);
      else { const uint8_t* p = si + 4 * (size_t)d; v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
    }
    di[d] = v;
  }
}
__global__ void __launch_bounds__(256) k_plonk_keys_scatter(const uint8_t* __restrict__ slot_status, const uint32_t* __restrict__ slot_to_proof, uint32_t m, uint32_t n_proofs,
                                                            uint8_t* __restrict__ status) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const uint32_t pi = slot_to_proof[j];
  if (pi < n_proofs) status[pi] = slot_status[j];
}

}  // namespace bn254

using namespace bn254;
hipError_t bn254_launch_plonk_keys_gather(const uint8_t* proofs, size_t stride, const uint8_t* inputs, size_t input_stride, uint32_t n_proofs, const uint32_t* slot_to_proof,
                                          const uint32_t* granule_key, const PlonkKeyDesc* desc, uint32_t n_keys, uint32_t m, uint8_t* recs, uint32_t rec_stride, uint32_t rec_bytes,
                                          uint8_t* rows, uint32_t row_stride, hipStream_t s) {
  hipLaunchKernelGGL(k_plonk_keys_gather, dim3((m + 3) / 4), dim3(256), 0, s, proofs, stride, inputs, input_stride, n_proofs, slot_to_proof, granule_key, desc, n_keys, m, recs,
                     rec_stride, rec_bytes, rows, row_stride);
  return hipGetLastError();
}
hipError_t bn254_launch_plonk_keys_scatter(const uint8_t* slot_status, const uint32_t* slot_to_proof, uint32_t m, uint32_t n_proofs, uint8_t* status, hipStream_t s) {
  hipLaunchKernelGGL(k_plonk_keys_scatter, dim3((m + 255) / 256), dim3(256), 0, s, slot_status, slot_to_proof, m, n_proofs, status);
  return hipGetLastError();
}
hipError_t bn254_launch_keys_group(const uint32_t* key_index, uint32_t n, uint32_t n_keys, uint32_t slot_cap, uint32_t* count, uint32_t* base, uint32_t* cursor,
                                   uint32_t* n_slots, uint32_t* slot_to_proof, uint32_t* granule_key, uint8_t* status, hipStream_t s) {
  hipError_t e;
  if ((e = hipMemsetAsync(count, 0, (size_t)n_keys * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(slot_to_proof, 0xff, (size_t)slot_cap * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(granule_key, 0, (size_t)(slot_cap / G16_KEYS_GRANULE + 1) * 4, s)) != hipSuccess) return e;
  const unsigned blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_keys_count, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, s, key_index, n, n_keys, count);
  hipLaunchKernelGGL(k_keys_scan, dim3(1), dim3(1024), 0, s, (const uint32_t*)count, n_keys, base, cursor, n_slots);
  hipLaunchKernelGGL(k_keys_place, dim3(blocks), dim3(256), 0, s, key_index, n, n_keys, cursor, slot_to_proof, granule_key, status);
  return hipGetLastError();
}
void bn254_launch_g16_prepare_keys(const G16KeysLaunchArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL(k_g16_prepare_keys, dim3(grid), dim3(256), 0, s, a.proofs, a.stride, a.inputs, a.input_stride, a.n_proofs, (uint32_t)a.m, a.slot0, a.n_slots, a.slot_to_proof,
                     a.granule_key, a.desc, a.n_keys, a.ws, a.slot_status);
  if (a.strict_scalars)
    hipLaunchKernelGGL(k_g16_check_scalars_keys, dim3(grid), dim3(256), 0, s, a.inputs, a.input_stride, a.n_proofs, (uint32_t)a.m, a.slot_to_proof, a.granule_key, a.desc, a.n_keys,
                       a.slot_status);
}
void bn254_launch_f12_mul_verdict_keys(const G16KeysLaunchArgs& a, unsigned grid, hipStream_t s, int e_dst, int e_a, int e_b) {
  hipLaunchKernelGGL(k_f12_mul_verdict_keys, dim3(grid), dim3(256), 0, s, a.ws, (uint32_t)a.m, (const uint8_t*)a.slot_status, a.slot_to_proof, a.granule_key, a.desc, a.n_keys,
                     a.n_proofs, a.status, e_dst, e_a, e_b);
}
