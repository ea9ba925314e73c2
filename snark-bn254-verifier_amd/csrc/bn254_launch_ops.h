// bn254_launch_ops.h -- what the units that launch the lane kernels share (hipcc only; bn254_kernels.hip, bn254_k_g16_load.hip, bn254_k_rlc.hip, bn254_k_probe.hip, and
// bn254_coop12.hip for the step table): the declarations of the kernels that more than one unit launches, the profile scope of a launch, the step-kind table of the
// Miller loop and LaunchOps, the host-side dispatcher of the VM programs (bn254_vm.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include "bn254_devws.h"

namespace bn254 {

// ---- kernels defined in one unit and launched from others (the __launch_bounds__ are the definitions') --------------------------------------------------------
// bn254_kernels.hip: one operation of the VM each; the subgroup test and the two compares
__global__ void k_vm_init(int32_t* ws, uint32_t n, const uint8_t* status);
__global__ void k_f12_sqr(int32_t* ws, uint32_t n, const uint8_t* status, int e);
__global__ void k_f12_mul_line_fixed(int32_t* ws, uint32_t n, const uint8_t* status, int e, const int32_t* entry, int e_px, int inf_mask);
__global__ void k_f12_mul_line_fixed2(int32_t* ws, uint32_t n, const uint8_t* status, int e, const int32_t* entry0, int e_px0, int inf_mask0, const int32_t* entry1, int e_px1,
                                      int inf_mask1);
__global__ void k_miller_dbl_var(int32_t* ws, uint32_t n, const uint8_t* status, int e_t, int e, int e_px);
__global__ void k_miller_sqr_dbl_var(int32_t* ws, uint32_t n, const uint8_t* status, int e_t, int e, int e_px);
__global__ void k_miller_add_var(int32_t* ws, uint32_t n, const uint8_t* status, int e_t, int e_b, int which, int e, int e_px);
__global__ void k_f12_mul(int32_t* ws, uint32_t n, const uint8_t* status, int d, int a, int b, int conj_b);
__global__ void k_f12_mul_verdict(int32_t* ws, uint32_t n, uint8_t* status, int d, int a, int b, const int32_t* target, int reject_code, const uint32_t* slot_proof,
                                  uint8_t* out_status);
__global__ void k_f12_copy(int32_t* ws, uint32_t n, const uint8_t* status, int d, int a);
__global__ void k_f12_cyclo_sqr(int32_t* ws, uint32_t n, const uint8_t* status, int d, int a);
__global__ void k_f12_cyclo_sqr_n(int32_t* ws, uint32_t n, const uint8_t* status, int d, int a, int count);
__global__ void k_f12_conj(int32_t* ws, uint32_t n, const uint8_t* status, int d, int a);
__global__ void k_f12_frob(int32_t* ws, uint32_t n, const uint8_t* status, int d, int a, int j);
__global__ void k_f12_inv(int32_t* ws, uint32_t n, const uint8_t* status, int d, int a);
__global__ void k_g16_compare(int32_t* ws, uint32_t n, uint8_t* status, const int32_t* target, int reject_code);
__global__ void k_g16_subgroup(uint32_t n, int32_t* ws, uint8_t* status, int inputs_match_key, int e_t);
// bn254_k_g16_load.hip: compaction, the loader, the strict-scalar check, the public-input MSM of keys with many inputs
__global__ void k_g16_classify(const uint8_t* proofs, size_t stride, uint32_t n, uint8_t* status, uint32_t* block_count);
__global__ void k_g16_compact_write(const uint8_t* status, uint32_t n, const uint32_t* block_count, uint32_t* slot_proof, uint8_t* slot_status);
__global__ void k_g16_prepare(const uint8_t* proofs, size_t stride, const uint8_t* inputs, int n_public, uint32_t n, int32_t* ws, uint8_t* status, const int32_t* msm_tab,
                              const int32_t* k0, int inputs_match_key, int wide_msm, const uint32_t* slot_proof, uint8_t* slot_status);
__global__ void k_g16_check_scalars(const uint8_t* inputs, int n_public, uint32_t n, uint8_t* status);
__global__ void k_g16_msm_partial(const uint8_t* inputs, int n_public, uint32_t n, int per, int chunks, const uint8_t* status, const int32_t* msm_tab, int32_t* part);
__global__ void k_g16_comb_digits(const uint8_t* inputs, int n_public, uint32_t n, uint16_t* digits);
__global__ void k_g16_msm_partial_comb(const uint16_t* digits, int n_public, uint32_t n, int per, int chunks, const uint8_t* status, const int32_t* msm_tab, int32_t* part);
__global__ void k_g16_msm_reduce(const int32_t* part, int chunks, uint32_t n, int32_t* ws, uint8_t* status, const int32_t* k0);
__global__ void k_g16_msm_reduce8(const int32_t* part, int chunks, uint32_t n, int32_t* ws, uint8_t* status, const int32_t* k0);

// ---- the 88 step kinds of the Miller loop (bn254_vm.h::miller_step_kind), built once: a byte per step, what vm_miller_program walks and the cooperative kernels read, and
// nibble-packed, what the run kernels take as an argument ---------------------------------------------------------------------------------------------------------
struct MillerStepTable { uint8_t kind[BN_ATE_STEPS]; MillerKinds packed; };
inline const MillerStepTable& miller_step_table() {
  static const MillerStepTable table = [] {
    MillerStepTable t;
    memset(&t, 0, sizeof t);
    for (int s = 0; s < BN_ATE_STEPS; s++) { t.kind[s] = (uint8_t)miller_step_kind(s); t.packed.nib[s >> 1] |= (uint8_t)(t.kind[s] << ((s & 1) * 4)); }
    return t;
  }();
  return table;
}

static inline unsigned grid_for(size_t n) { return (unsigned)((n + 255) / 256); }
struct ProfScope {  // records the event pair around one launch (no-op without a profile or for unselected kinds)
  G16Prof* p; hipStream_t s; int slot;
  ProfScope(G16Prof* p_, int kid, hipStream_t s_) : p(p_), s(s_), slot(-1) {
    if (p && ((p->mask >> kid) & 1u) && p->used < p->cap) { slot = p->used++; p->kid[slot] = (uint8_t)kid; (void)hipEventRecord(p->ev[2 * slot], s); }
  }
  ~ProfScope() { if (slot >= 0) (void)hipEventRecord(p->ev[2 * slot + 1], s); }
};
#define BN_LAUNCH(KID, KERNEL, ...) do { ProfScope ps_(prof, KID, s); hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(256), 0, s, __VA_ARGS__); } while (0)
// host-side OPS for the VM programs: every operation is one kernel launch on the stream
struct LaunchOps {
  int32_t* ws; uint32_t n; const uint8_t* status; unsigned grid; hipStream_t s;
  const int32_t* tab[3];
  G16Prof* prof;
  int inf_mask[3] = {BN254_ST_LINF, 0, 0};   // status bits marking the G1 point of fixed pair 0 / 1 / 2 as the identity
  const G16KeyDesc* key_desc = nullptr; uint32_t n_keys = 0; const uint32_t* granule_key = nullptr;   // a batch over many keys: miller_run reads the tables per wavefront
  const PlonkKeyDesc* plonk_desc = nullptr;  // a PlonK batch over many keys: miller_run_fixed2 reads the tables per wavefront (n_keys, granule_key as above)
  int run_fold = 0, inputs_match_key = 0;    // miller_run: MR_FOLD_INIT | MR_FOLD_ATE (the first run sets f and T, the last one tests B's subgroup and writes status)
  int uni(int x) { return x; }
  void f12_sqr(int e) { BN_LAUNCH(KID_F12_SQR, k_f12_sqr, ws, n, status, e); }
  void miller_dbl_var(int et, int e, int ep) { BN_LAUNCH(KID_MILLER_DBL_VAR, k_miller_dbl_var, ws, n, status, et, e, ep); }
  void miller_step(bool do_sqr, int kind, int st_, int et, int eb, int e, int epa, int ep0, int ep1) {
    const int32_t *t0 = tab[0] + (size_t)st_ * FIXED_LINE_DWORDS, *t1 = tab[1] + (size_t)st_ * FIXED_LINE_DWORDS;
    ProfScope ps_(prof, kind == 0 ? KID_MILLER_STEP_DBL : KID_MILLER_STEP_ADD, s);
    bn254_launch_miller_step(do_sqr, kind, ws, n, status, grid, s, et, eb, e, epa, t0, ep0, inf_mask[0], t1, ep1, inf_mask[1]);
  }
  void miller_run(int s_begin, int s_end, int et, int eb, int e, int epa, int ep0, int ep1) {
    const MillerKinds& kinds = miller_step_table().packed;
    ProfScope ps_(prof, KID_MILLER_RUN, s);
    if (key_desc) { bn254_launch_miller_run_keys(kinds, s_begin, s_end, ws, n, (uint8_t*)status, grid, s, et, eb, e, epa, key_desc, n_keys, granule_key, ep0, inf_mask[0], ep1, inf_mask[1], run_fold); return; }
    bn254_launch_miller_run(kinds, s_begin, s_end, ws, n, (uint8_t*)status, grid, s, et, eb, e, epa, tab[0], ep0, inf_mask[0], tab[1], ep1, inf_mask[1], run_fold, inputs_match_key);
  }
  void miller_run_fixed2(int s_begin, int s_end, int e, int ep0, int ep1) {
    const MillerKinds& kinds = miller_step_table().packed;
    ProfScope ps_(prof, KID_MILLER_RUN, s);
    if (plonk_desc) { bn254_launch_miller_run_fixed2_keys(kinds, s_begin, s_end, ws, n, status, grid, s, e, plonk_desc, n_keys, granule_key, ep0, inf_mask[0], ep1, inf_mask[1]); return; }
    bn254_launch_miller_run_fixed2(kinds, s_begin, s_end, ws, n, status, grid, s, e, tab[0], ep0, inf_mask[0], tab[1], ep1, inf_mask[1]);
  }
  void miller_sqr_dbl_var(int et, int e, int ep) { BN_LAUNCH(KID_MILLER_SQR_DBL_VAR, k_miller_sqr_dbl_var, ws, n, status, et, e, ep); }
  void miller_add_var(int et, int eb, int which, int e, int ep) { BN_LAUNCH(KID_MILLER_ADD_VAR, k_miller_add_var, ws, n, status, et, eb, which, e, ep); }
  void f12_mul_line_fixed(int e, int t, int st_, int ep) {
    BN_LAUNCH(KID_MUL_LINE_FIXED, k_f12_mul_line_fixed, ws, n, status, e, tab[t] + (size_t)st_ * FIXED_LINE_DWORDS, ep, inf_mask[t]);
  }
  void f12_mul_line_fixed2(int e, int st_, int ep0, int ep1) {
    BN_LAUNCH(KID_MUL_LINE_FIXED2, k_f12_mul_line_fixed2, ws, n, status, e, tab[0] + (size_t)st_ * FIXED_LINE_DWORDS, ep0, inf_mask[0],
              tab[1] + (size_t)st_ * FIXED_LINE_DWORDS, ep1, inf_mask[1]);
  }
  void f12_mul(int d, int a, int b, bool conj_b = false) { BN_LAUNCH(KID_F12_MUL, k_f12_mul, ws, n, status, d, a, b, conj_b ? 1 : 0); }
  void f12_copy(int d, int a) { BN_LAUNCH(KID_F12_COPY, k_f12_copy, ws, n, status, d, a); }
  void f12_cyclo_sqr(int d, int a) { BN_LAUNCH(KID_CYCLO_SQR, k_f12_cyclo_sqr, ws, n, status, d, a); }
  void f12_cyclo_sqr_n(int d, int a, int count) { BN_LAUNCH(KID_CYCLO_SQR_N, k_f12_cyclo_sqr_n, ws, n, status, d, a, count); }
  void f12_conj(int d, int a) { BN_LAUNCH(KID_F12_CONJ, k_f12_conj, ws, n, status, d, a); }
  void f12_frob(int d, int a, int j) { BN_LAUNCH(KID_F12_FROB, k_f12_frob, ws, n, status, d, a, j); }
  void f12_inv(int d, int a) { BN_LAUNCH(KID_F12_INV, k_f12_inv, ws, n, status, d, a); }
};

}  // namespace bn254
