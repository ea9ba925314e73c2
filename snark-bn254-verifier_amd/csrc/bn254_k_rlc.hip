// bn254_k_rlc.hip -- the random-linear-combination batch mode of Groth16 (bn254_rlc.h): the workspace accessors of the fold (DevWs2) and of the shared-accumulator
// Miller loop (DevWsM), the k_rlc_* kernels and bn254_launch_g16_rlc, which enqueues one launch part: per-proof stage, fold, group stage, scatter.  The loader, the
// MSM kernels of wide keys and the one-operation VM kernels it launches are the exact path's (bn254_launch_ops.h).
#include <hip/hip_runtime.h>
#include "bn254_launch_ops.h"
#include "bn254_rlc.h"

namespace bn254 {

// =====================================================================================================================
// random-linear-combination batch mode (bn254_rlc.h)
// =====================================================================================================================
// accessor of the fold: element ids >= RLC_HI address the partner lane's column of the same workspace
struct DevWs2 {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t row_bytes, voff_lo, voff_hi;
  int32_t* lds;
  __device__ __forceinline__ DevWs2(int32_t* base, uint32_t n, uint32_t lane_lo, uint32_t lane_hi, int32_t* lds_) : lds(lds_) {
    DevWs t(base, n, lane_lo);
    rsrc = t.rsrc; row_bytes = t.row_bytes; voff_lo = lane_lo * 4u; voff_hi = lane_hi * 4u;
  }
  __device__ __forceinline__ void park(int slot, const Fp2& a) const {
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { lds[(slot * 18 + l) * 256 + threadIdx.x] = a.c0.v[l]; lds[(slot * 18 + BN_NL + l) * 256 + threadIdx.x] = a.c1.v[l]; }
  }
  __device__ __forceinline__ Fp2 unpark(int slot) const {
    Fp2 r;
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { r.c0.v[l] = lds[(slot * 18 + l) * 256 + threadIdx.x]; r.c1.v[l] = lds[(slot * 18 + BN_NL + l) * 256 + threadIdx.x]; }
    return r;
  }
  __device__ __forceinline__ Fp ld(int e) const {
    Fp r;
    uint32_t eu = __builtin_amdgcn_readfirstlane((uint32_t)e);
    const bool hi = eu >= (uint32_t)RLC_HI;   // wave-uniform
    if (hi) eu -= (uint32_t)RLC_HI;
    const uint32_t vo = hi ? voff_hi : voff_lo;
#pragma unroll
    for (int l = 0; l < BN_NL; l++) r.v[l] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, vo, (eu * (uint32_t)BN_NL + (uint32_t)l) * row_bytes, 0);
    return r;
  }
  __device__ __forceinline__ void st(int e, const Fp& a) const {
    uint32_t eu = __builtin_amdgcn_readfirstlane((uint32_t)e);
#pragma unroll
    for (int l = 0; l < BN_NL; l++) __builtin_amdgcn_raw_buffer_store_b32(a.v[l], rsrc, voff_lo, (eu * (uint32_t)BN_NL + (uint32_t)l) * row_bytes, 0);
  }
};
// accessor of the shared-accumulator Miller loop: the lane's own column (f) and the column of the current proof (sel(q): lane + q * m)
struct DevWsM {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t row_bytes, voff0, lane, m, n, voff;
  int32_t* lds;
  __device__ __forceinline__ DevWsM(int32_t* base, uint32_t n_, uint32_t lane_, uint32_t m_, int32_t* lds_) : lane(lane_), m(m_), n(n_), lds(lds_) {
    DevWs t(base, n_, lane_);
    rsrc = t.rsrc; row_bytes = t.row_bytes; voff0 = lane_ < n_ ? lane_ * 4u : 0xfffffffcu; voff = voff0;
  }
  __device__ __forceinline__ void sel(int q) { const uint32_t i = lane + (uint32_t)q * m; voff = (lane < m && i < n) ? i * 4u : 0xfffffffcu; }
  __device__ __forceinline__ void park(int slot, const Fp2& a) const {
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { lds[(slot * 18 + l) * 256 + threadIdx.x] = a.c0.v[l]; lds[(slot * 18 + BN_NL + l) * 256 + threadIdx.x] = a.c1.v[l]; }
  }
  __device__ __forceinline__ Fp2 unpark(int slot) const {
    Fp2 r;
#pragma unroll
    for (int l = 0; l < BN_NL; l++) { r.c0.v[l] = lds[(slot * 18 + l) * 256 + threadIdx.x]; r.c1.v[l] = lds[(slot * 18 + BN_NL + l) * 256 + threadIdx.x]; }
    return r;
  }
  __device__ __forceinline__ Fp ldv(int e, uint32_t vo) const {
    Fp r;
    uint32_t eu = __builtin_amdgcn_readfirstlane((uint32_t)e);
#pragma unroll
    for (int l = 0; l < BN_NL; l++) r.v[l] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, vo, (eu * (uint32_t)BN_NL + (uint32_t)l) * row_bytes, 0);
    return r;
  }
  __device__ __forceinline__ void stv(int e, const Fp& a, uint32_t vo) const {
    uint32_t eu = __builtin_amdgcn_readfirstlane((uint32_t)e);
#pragma unroll
    for (int l = 0; l < BN_NL; l++) __builtin_amdgcn_raw_buffer_store_b32(a.v[l], rsrc, vo, (eu * (uint32_t)BN_NL + (uint32_t)l) * row_bytes, 0);
  }
  __device__ __forceinline__ Fp ld(int e) const { return ldv(e, voff); }
  __device__ __forceinline__ void st(int e, const Fp& a) const { stv(e, a, voff); }
  __device__ __forceinline__ Fp ld0(int e) const { return ldv(e, voff0); }
  __device__ __forceinline__ void st0(int e, const Fp& a) const { stv(e, a, voff0); }
};
// one Miller step of the G proofs of a lane with a shared accumulator (bn254_rlc.h::vm_miller_var_multi); lanes [0, m)
template <bool DO_SQR>
__global__ void __launch_bounds__(256, 2)
k_rlc_miller_multi(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int kind, int G, uint32_t m) {
  __shared__ int32_t park_lds[72 * 256];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  uint32_t deadmask = 0;
  const int g = __builtin_amdgcn_readfirstlane(G);
  for (int q = 0; q < g; q++) {
    const uint32_t i = j + (uint32_t)q * m;
    const bool live = j < m && i < n && (status[i < n ? i : n - 1] & BN254_ST_PENDING) != 0;
    if (!live) deadmask |= 1u << q;
  }
  if (__builtin_amdgcn_ballot_w64(j < m) == 0) return;
  DevWsM w(ws, n, j < m ? j : 0xffffffffu, m, park_lds);
  vm_miller_var_multi<DO_SQR>(w, __builtin_amdgcn_readfirstlane(kind), g, deadmask);
}
// f = 1 on the lanes that carry an accumulator; T = B on every pending proof (k_vm_init does both for the one-proof-per-lane layout)
__global__ void __launch_bounds__(256, 2) k_rlc_init_f(int32_t* ws, uint32_t n, uint32_t m) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  DevWs w(ws, n, j < m ? j : DEAD_LANE);
  w.st(VE_F, fp_one());
  for (int e = 1; e < 12; e++) w.st(VE_F + e, fp_zero());
}
// per pending proof: weight r_i = ChaCha20(key, counter_base + i), A <- r A, C' <- r C, t_j = r x_j (bn254_rlc.h::vm_rlc_scale)
__global__ void __launch_bounds__(256, 2)
k_rlc_scale(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, const uint8_t* __restrict__ inputs, int n_public, ChaChaKey key, uint32_t counter_base) {
  VM_KERNEL_PROLOGUE();
  const uint32_t ii = i < n ? i : n - 1;
  uint32_t r[4];
  chacha20_block4(r, key, counter_base + ii);
  const uint8_t* in = inputs + (size_t)ii * (size_t)n_public * 32;
  vm_rlc_scale(w, r, n_public, [&](int j, uint32_t* o) { words_from_be(o, in + 32 * j); });
}
// lanes that are no longer pending contribute the neutral element to their group
__global__ void __launch_bounds__(256, 2)
k_rlc_neutral(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int n_public, int with_f) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool dead = i < n && (status[i] & BN254_ST_PENDING) == 0;
  if (__builtin_amdgcn_ballot_w64(dead) == 0) return;
  DevWs w(ws, n, dead ? i : DEAD_LANE);
  vm_rlc_neutral(w, n_public, __builtin_amdgcn_readfirstlane(with_f) != 0);
}
// one fold round: lane j < cur - half takes lane j + half (bn254_rlc.h::vm_rlc_fold)
__global__ void __launch_bounds__(256, 2)
k_rlc_fold(int32_t* ws, uint32_t n, uint32_t cur, uint32_t half, int n_public, int with_f) {
  __shared__ int32_t park_lds[72 * 256];
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const bool act = j + half < cur;
  if (__builtin_amdgcn_ballot_w64(act) == 0) return;
  DevWs2 w(ws, n, act ? j : DEAD_LANE, act ? j + half : DEAD_LANE, park_lds);
  vm_rlc_fold(w, n_public, __builtin_amdgcn_readfirstlane(with_f) != 0);
}
// group stage, one lane per group: the G1 arguments of the three table-driven pairs (bn254_rlc.h::vm_rlc_group_points)
__global__ void __launch_bounds__(256, 2)
k_rlc_group_points(int32_t* ws, uint32_t n, uint8_t* __restrict__ grp_status, uint32_t groups, int n_public, const int32_t* __restrict__ rlc_tab,
                   const int32_t* __restrict__ msm_tab) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (__builtin_amdgcn_ballot_w64(g < groups) == 0) return;
  DevWs w(ws, n, g < groups ? g : DEAD_LANE);
  const int fl = vm_rlc_group_points(w, n_public, [&](int b, int wi, int d) {
    return b < 2 ? msm_entry(rlc_tab, (size_t)(b * MSM_FW_WINDOWS + wi) * MSM_FW_ENTRIES + d) : msm_entry(msm_tab, (size_t)((b - 2) * MSM_FW_WINDOWS + wi) * MSM_FW_ENTRIES + d);
  });
  if (g < groups) grp_status[g] = (uint8_t)(BN254_ST_PENDING | ((fl & 1) ? BN254_ST_LINF : 0) | ((fl & 2) ? BN254_ST_LINF2 : 0) | ((fl & 4) ? BN254_ST_LINF3 : 0));
}
// group stage: one Miller step of the three table-driven pairs (bn254_rlc.h::vm_miller_step_fixed3)
template <bool DO_SQR>
__global__ void __launch_bounds__(256, 2)
k_rlc_group_step(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e, const int32_t* __restrict__ entry0, const int32_t* __restrict__ entry1,
                 const int32_t* __restrict__ entry2) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  FixedLine l0, l1, l2;
  l0.m = uni_ld2(entry0); l0.c = uni_ld2(entry0 + 2 * BN_NL); l0.xc = uni_ld2(entry0 + 4 * BN_NL);
  l1.m = uni_ld2(entry1); l1.c = uni_ld2(entry1 + 2 * BN_NL); l1.xc = uni_ld2(entry1 + 4 * BN_NL);
  l2.m = uni_ld2(entry2); l2.c = uni_ld2(entry2 + 2 * BN_NL); l2.xc = uni_ld2(entry2 + 4 * BN_NL);
  vm_miller_step_fixed3<DO_SQR>(w, e, l0, VE_LX, (st & BN254_ST_LINF) != 0, l1, VE_CX, (st & BN254_ST_LINF2) != 0, l2, VE_AX, (st & BN254_ST_LINF3) != 0);
}
// ---- wide keys (n_public > RLC_MAX_PUBLIC, bn254_rlc.h): t_0 = r_i per proof, the public-input sum once per group from the group scalars --------------
// per pending proof: as k_rlc_scale without the n_public products; the weight's halves k1 | k2 go to RLC_W for k_rlc_group_scalars
__global__ void __launch_bounds__(256, 2)
k_rlc_scale_wide(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, ChaChaKey key, uint32_t counter_base) {
  VM_KERNEL_PROLOGUE();
  const uint32_t ii = i < n ? i : n - 1;
  uint32_t r[4];
  chacha20_block4(r, key, counter_base + ii);
  vm_rlc_scale(w, r, 0, [&](int, uint32_t*) {});
  Fr8 k = fr8_zero();
#pragma unroll
  for (int q = 0; q < 4; q++) k.w[q] = r[q];
  w.st(RLC_W, fr8_to_slot(k));
}
// s_gj = sum_{i in g} r_i x_ij mod r (bn254_rlc.h::rlc_group_scalar), lane t = g * n_public + j: the lanes of a wavefront read consecutive 32-byte inputs of a
// member's row (contiguous over j; a wavefront spans one or two groups, whose members are walked in the same order), and write the group's row of scalars
// rows[(g * n_public + j) * 32] -- big-endian, the layout of the batch's own input rows -- contiguously.  A proof that is no longer pending (loader error, r-torsion
// failure, STRICT_SCALARS) has weight 0, as k_rlc_neutral gives its t_0.
__global__ void __launch_bounds__(256)
k_rlc_group_scalars(const int32_t* __restrict__ ws, uint32_t n, const uint8_t* __restrict__ status, const uint8_t* __restrict__ inputs, int n_public, RlcPlan plan,
                    uint8_t* __restrict__ rows) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= plan.groups * (uint32_t)n_public) return;
  const uint32_t g = t / (uint32_t)n_public;
  const int j = (int)(t - g * (uint32_t)n_public);
  const bool aligned = (((uintptr_t)inputs) & 3) == 0;
  const Fr8 s = rlc_group_scalar(g, j, n, plan,
      [&](uint32_t i, int jj, uint32_t x[8]) {
        const uint8_t* sp = inputs + ((size_t)i * (size_t)n_public + (size_t)jj) * 32;
        if (aligned) { uint32_t d[8];
#pragma unroll
          for (int k = 0; k < 8; k++) d[k] = ((const uint32_t*)sp)[k];
          be_field_to_words(x, d);
        } else words_from_be(x, sp);
      },
      [&](uint32_t i, uint32_t k[4]) -> bool {
        if (!(status[i] & BN254_ST_PENDING)) return false;
#pragma unroll
        for (int q = 0; q < 4; q++) k[q] = (uint32_t)ws[((size_t)RLC_W * BN_NL + q) * n + i];
        return true;
      });
  words_to_be(rows + (size_t)t * 32, s.w);
}
// group stage of a wide key, one lane per group (bn254_rlc.h::vm_rlc_group_points_wide).  form 2 (up to 16 inputs): sum_j s_j K_j from the key's 13-bit window
// tables and the group's row of scalars; forms 0 / 1: the chunk sums k_g16_msm_partial(_comb) left in `part` for the group "pseudo-proofs" (no K_0 there)
__global__ void __launch_bounds__(256, 2)
k_rlc_group_points_wide(int32_t* ws, uint32_t n, uint8_t* __restrict__ grp_status, uint32_t groups, int n_public, const int32_t* __restrict__ rlc_tab,
                        const int32_t* __restrict__ msm_tab, const uint8_t* __restrict__ rows, const int32_t* __restrict__ part, int chunks, int form) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (__builtin_amdgcn_ballot_w64(g < groups) == 0) return;
  const uint32_t gg = g < groups ? g : groups - 1;
  DevWs w(ws, n, g < groups ? g : DEAD_LANE);
  G1Proj Lk = g1_identity();
  if (__builtin_amdgcn_readfirstlane(form) == 2) {
    for (int j = 0; j < n_public; j++) {
      Fr8 sj;
      words_from_be(sj.w, rows + ((size_t)gg * (size_t)n_public + (size_t)j) * 32);
      Lk = g1_window_sum(Lk, sj, [&](int wi, int d) { return msm_entry(msm_tab, (size_t)(j * MSM_FW_WINDOWS + wi) * MSM_FW_ENTRIES + d); });
    }
  } else {
    for (int c = 0; c < chunks; c++) {
      const int32_t* o = part + (size_t)c * 27 * groups + gg;
      G1Proj q;
#pragma unroll
      for (int l = 0; l < BN_NL; l++) { q.x.v[l] = o[(size_t)l * groups]; q.y.v[l] = o[(size_t)(9 + l) * groups]; q.z.v[l] = o[(size_t)(18 + l) * groups]; }
      BN_SETB(q.x, 3.0, 0.5); BN_SETB(q.y, 3.0, 0.5); BN_SETB(q.z, 3.0, 0.5);
      Lk = g1_add(Lk, q);
    }
    Lk.x = fp_reduce(Lk.x); Lk.y = fp_reduce(Lk.y); Lk.z = fp_reduce(Lk.z);
    BN_SETB(Lk.x, 1.01, 0.5); BN_SETB(Lk.y, 1.01, 0.5); BN_SETB(Lk.z, 1.01, 0.5);
  }
  const int fl = vm_rlc_group_points_wide(w, Lk, [&](int b, int wi, int d) { return msm_entry(rlc_tab, (size_t)(b * MSM_FW_WINDOWS + wi) * MSM_FW_ENTRIES + d); });
  if (g < groups) grp_status[g] = (uint8_t)(BN254_ST_PENDING | ((fl & 1) ? BN254_ST_LINF : 0) | ((fl & 2) ? BN254_ST_LINF2 : 0) | ((fl & 4) ? BN254_ST_LINF3 : 0));
}
// every pending proof takes its group's verdict: ACCEPT, or it stays pending (0x80) for the exact path
__global__ void __launch_bounds__(256, 2)
k_rlc_scatter(uint8_t* __restrict__ status, uint32_t n, const uint8_t* __restrict__ grp_status, RlcPlan plan) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = status[i];
  if (!(st & BN254_ST_PENDING)) return;
  status[i] = grp_status[rlc_group_of(i, plan)] == BN254_ST_ACCEPT ? (uint8_t)BN254_ST_ACCEPT : (uint8_t)BN254_ST_PENDING;
}

}  // namespace bn254

using namespace bn254;
// ---- RLC batch mode: per-proof stage, fold, group stage, scatter (bn254_rlc.h; orchestration of the fallback in bn254_capi.hip) ---------------------
hipError_t bn254_launch_g16_rlc(const G16LaunchArgs& a, const RlcLaunchArgs& r, hipStream_t s) {
  unsigned grid = grid_for(a.n);
  uint32_t n = (uint32_t)a.n;
  G16Prof* prof = nullptr;
  ChaChaKey key;
  for (int i = 0; i < 8; i++) key.k[i] = r.key[i];
  for (int i = 0; i < 3; i++) key.nonce[i] = r.key[8 + i];
  // parse + checks; the public-input MSM is skipped (done once per group): the wide flag of k_g16_prepare returns before it
  BN_LAUNCH(KID_PREPARE, k_g16_prepare, a.proofs, a.stride, a.inputs, a.n_public, n, a.ws, a.status, a.msm_tab, a.k0, a.inputs_match_key, 1, (const uint32_t*)nullptr, (uint8_t*)nullptr);
  if (a.strict_scalars && a.n_public > 0) hipLaunchKernelGGL(k_g16_check_scalars, dim3(grid), dim3(256), 0, s, a.inputs, a.n_public, n, a.status);
  LaunchOps ops{a.ws, n, a.status, grid, s, {nullptr, nullptr, nullptr}, nullptr};
  BN_LAUNCH(KID_VM_INIT, k_vm_init, a.ws, n, (const uint8_t*)a.status);
  // wide keys carry t_0 alone through the fold (slots: the Fr values per lane), their group scalars come from k_rlc_group_scalars
  const bool wide = r.grp_rows != nullptr;
  const int slots = wide ? 0 : a.n_public;
  if (wide) hipLaunchKernelGGL(k_rlc_scale_wide, dim3(grid), dim3(256), 0, s, a.ws, n, (const uint8_t*)a.status, key, r.counter_base);
  else hipLaunchKernelGGL(k_rlc_scale, dim3(grid), dim3(256), 0, s, a.ws, n, (const uint8_t*)a.status, a.inputs, a.n_public, key, r.counter_base);
  const uint8_t* kinds = miller_step_table().kind;
  const int share = 1 << r.plan.pre;
  if (share == 1) {
    vm_miller_program(ops, kinds, false);
  } else {
    // shared accumulators: lane j < m walks proofs j, j + m, ..., j + (share - 1) m; one squaring of f per lane and step
    const uint32_t m = r.plan.lanes;
    const unsigned mgrid = grid_for(m);
    hipLaunchKernelGGL(k_rlc_init_f, dim3(mgrid), dim3(256), 0, s, a.ws, n, m);
    for (int st_ = 0; st_ < BN_ATE_STEPS; st_++) {
      const int kind = kinds[st_];
      if (kind == 0 && st_ != 0) hipLaunchKernelGGL(k_rlc_miller_multi<true>, dim3(mgrid), dim3(256), 0, s, a.ws, n, (const uint8_t*)a.status, kind, share, m);
      else hipLaunchKernelGGL(k_rlc_miller_multi<false>, dim3(mgrid), dim3(256), 0, s, a.ws, n, (const uint8_t*)a.status, kind, share, m);
    }
  }
  BN_LAUNCH(KID_SUBGROUP, k_g16_subgroup, n, a.ws, a.status, a.inputs_match_key, (int)VE_T);
  hipLaunchKernelGGL(k_rlc_neutral, dim3(grid), dim3(256), 0, s, a.ws, n, (const uint8_t*)a.status, slots, share == 1 ? 1 : 0);
  uint32_t cur = n;
  for (int k = 0; k < r.plan.rounds; k++) {
    const uint32_t half = r.plan.half[k];
    hipLaunchKernelGGL(k_rlc_fold, dim3(grid_for(cur - half)), dim3(256), 0, s, a.ws, n, cur, half, slots, k >= r.plan.pre ? 1 : 0);
    cur = half;
  }
  // group stage: lanes [0, groups) of the same workspace, their own status bytes
  const uint32_t groups = r.plan.groups;
  const unsigned ggrid = grid_for(groups);
  if (wide) {
    // the group scalars become the input rows of `groups` pseudo-proofs: the key's own fixed-base kernels sum them (no K_0: vm_rlc_group_points_wide adds t_0 K_0)
    const size_t lanes = (size_t)groups * (size_t)a.n_public;
    hipLaunchKernelGGL(k_rlc_group_scalars, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, (const int32_t*)a.ws, n, (const uint8_t*)a.status, a.inputs, a.n_public, r.plan, r.grp_rows);
    (void)hipMemsetAsync(r.grp_status, BN254_ST_PENDING, ((size_t)groups + 255) / 256 * 256, s);    // every pseudo-proof takes part in the partial sums
    const int per = G16_WIDE_MSM_INPUTS_PER_LANE, chunks = r.msm_form == 2 ? 0 : (a.n_public + per - 1) / per;
    const unsigned pg = (unsigned)(((size_t)groups * chunks + 255) / 256);
    if (r.msm_form == 0) {
      hipLaunchKernelGGL(k_g16_comb_digits, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, (const uint8_t*)r.grp_rows, a.n_public, groups, r.grp_digits);
      hipLaunchKernelGGL(k_g16_msm_partial_comb, dim3(pg), dim3(256), 0, s, (const uint16_t*)r.grp_digits, a.n_public, groups, per, chunks, (const uint8_t*)r.grp_status, a.msm_tab, r.grp_part);
    } else if (r.msm_form == 1) {
      hipLaunchKernelGGL(k_g16_msm_partial, dim3(pg), dim3(256), 0, s, (const uint8_t*)r.grp_rows, a.n_public, groups, per, chunks, (const uint8_t*)r.grp_status, a.msm_tab, r.grp_part);
    }
    hipLaunchKernelGGL(k_rlc_group_points_wide, dim3(ggrid), dim3(256), 0, s, a.ws, n, r.grp_status, groups, a.n_public, r.rlc_tab, a.msm_tab, (const uint8_t*)r.grp_rows,
                       (const int32_t*)r.grp_part, chunks, r.msm_form);
  } else {
    (void)hipMemsetAsync(r.grp_status, 0, ((size_t)groups + 255) / 256 * 256, s);
    hipLaunchKernelGGL(k_rlc_group_points, dim3(ggrid), dim3(256), 0, s, a.ws, n, r.grp_status, groups, a.n_public, r.rlc_tab, a.msm_tab);
  }
  LaunchOps gops{a.ws, n, r.grp_status, ggrid, s, {a.gtab, a.dtab, r.btab}, nullptr};
  gops.inf_mask[0] = BN254_ST_LINF; gops.inf_mask[1] = BN254_ST_LINF2; gops.inf_mask[2] = BN254_ST_LINF3;
  for (int st_ = 0; st_ < BN_ATE_STEPS; st_++) {
    const int32_t *t0 = a.gtab + (size_t)st_ * FIXED_LINE_DWORDS, *t1 = a.dtab + (size_t)st_ * FIXED_LINE_DWORDS, *t2 = r.btab + (size_t)st_ * FIXED_LINE_DWORDS;
    if (kinds[st_] == 0 && st_ != 0) hipLaunchKernelGGL(k_rlc_group_step<true>, dim3(ggrid), dim3(256), 0, s, a.ws, n, (const uint8_t*)r.grp_status, (int)RLC_ACC, t0, t1, t2);
    else hipLaunchKernelGGL(k_rlc_group_step<false>, dim3(ggrid), dim3(256), 0, s, a.ws, n, (const uint8_t*)r.grp_status, (int)RLC_ACC, t0, t1, t2);
  }
  gops.f12_mul(VE_F, VE_F, RLC_ACC);
  vm_final_exp_program(gops);
  { unsigned grid = ggrid; BN_LAUNCH(KID_COMPARE, k_g16_compare, a.ws, n, r.grp_status, r.one, BN254_ST_REJECT); }
  hipLaunchKernelGGL(k_rlc_scatter, dim3(grid), dim3(256), 0, s, a.status, n, (const uint8_t*)r.grp_status, r.plan);
  return hipGetLastError();
}
