// bn254_kernels.hip -- the one-operation kernels of the verification VM (bn254_vm.h), one proof per lane, and the launchers that walk its programs: an exact Groth16
// batch under one key (bn254_launch_g16), over a key list in slots (bn254_launch_g16_keys) or directly (bn254_launch_g16_keys_direct), and PlonK's two-pair
// pairing check (bn254_launch_pairing2_fixed*).  Beside it: the loader and the wide MSM in bn254_k_g16_load.hip, the RLC mode in bn254_k_rlc.hip, the probes in
// bn254_k_probe.hip; what the four share -- LaunchOps, the kernels' declarations -- in bn254_launch_ops.h.
//
// Pipeline of an exact Groth16 batch (DESIGN.md "Kernels"):
//   k_g16_prepare (bn254_k_g16_load.hip)
//                     parse 256 proof bytes (coalesced through LDS), range / on-curve checks of A, B, C, Montgomery
//                     conversion, L = K0 + sum x_i K_i by fixed-base windows (bn254_fw.h)       (groth16/converter.rs:14-26, verify.rs:53-63)
//   k_miller_run (bn254_k_miller.hip)
//                     the shared Miller loop f = Miller(A,B) * lines_G(L) * lines_D(C) in runs of steps, by default ONE launch
//                     (bn254_vm.h::vm_miller_run); G/D line tables shared by the batch.  The first launch sets f = 1, T = (B, 1);
//                     the last one ends with the r-torsion test of B on the loop's final G2 point and the status precedence
//                                                                                               (verify.rs:73-77, converter.rs:152)
//   k_f12_inv, k_f12_frob, k_f12_mul, k_f12_cyclo_sqr(_n)
//                     f^((p^12-1)/r), bn254_vm.h::vm_final_exp_program: conjugations ride on their consumers' loads (verify.rs:77)
//   k_f12_mul_verdict the program's last product, compared == e(alpha, beta) as it is stored -> status byte   (verify.rs:77)
// The latency mode and the one-launch-per-step form (k_miller_step_dbl / _add, k_miller_*_var) keep k_vm_init, k_g16_subgroup and
// k_g16_compare as launches of their own; so does the RLC mode.
//
// Every operation of the VM is its own kernel: it gets the full 256-VGPR budget of a 2-waves-per-SIMD launch and keeps nothing in registers between
// operations (the workspace they meet in: bn254_devws.h).  The host walks a program through LaunchOps and enqueues one launch per operation; in the throughput
// form the Miller loop is no program walk but k_miller_run launches, and what is walked is the final exponentiation.
#include <hip/hip_runtime.h>
#include "bn254_launch_ops.h"
#include "bn254_g16_plan.h"

static_assert(G16_MILLER_STEPS == BN_ATE_STEPS, "bn254_g16_plan.h counts the Miller steps of bn254_constants.h");

namespace bn254 {
// Compiled twice (Makefile): the first object holds everything but the body of k_f12_mul_verdict; the second (-DBN_PLAIN_HALF -DBN_NO_CARRY_RIDE) holds only that kernel,
// which keeps the reassociated carry chains: with the carry ride it spills more (profiles/carry_chain_resources.txt).
#ifndef BN_PLAIN_HALF

__global__ void __launch_bounds__(256, 2) k_vm_init(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status) {  // f = 1, T = B
  VM_KERNEL_PROLOGUE();
  w.st(VE_F, fp_one());
  for (int e = 1; e < 12; e++) w.st(VE_F + e, fp_zero());
  for (int e = 0; e < 4; e++) w.st(VE_T + e, w.ld(VE_B + e));
  w.st(VE_T + 4, fp_one()); w.st(VE_T + 5, fp_zero());
}
__global__ void __launch_bounds__(256, 2) k_f12_sqr(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e) { VM_KERNEL_PROLOGUE(); vm_f12_sqr(w, e); }
__global__ void __launch_bounds__(256, 2) k_f12_mul_line_fixed(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e, const int32_t* __restrict__ entry, int e_px, int inf_mask) {
  VM_KERNEL_PROLOGUE();
  FixedLine l; l.m = uni_ld2(entry); l.c = uni_ld2(entry + 2 * BN_NL); l.xc = uni_ld2(entry + 4 * BN_NL);
  vm_f12_mul_line_fixed(w, e, l, e_px, (st & inf_mask) != 0);  // inf_mask: the status bit that marks this pair's G1 point as the identity
}
__global__ void __launch_bounds__(256, 2) k_f12_mul_line_fixed2(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e, const int32_t* __restrict__ entry0,
                                                                int e_px0, int inf_mask0, const int32_t* __restrict__ entry1, int e_px1, int inf_mask1) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  FixedLine l0, l1;
  l0.m = uni_ld2(entry0); l0.c = uni_ld2(entry0 + 2 * BN_NL); l0.xc = uni_ld2(entry0 + 4 * BN_NL);
  l1.m = uni_ld2(entry1); l1.c = uni_ld2(entry1 + 2 * BN_NL); l1.xc = uni_ld2(entry1 + 4 * BN_NL);
  vm_f12_mul_line_fixed2(w, e, l0, e_px0, (st & inf_mask0) != 0, l1, e_px1, (st & inf_mask1) != 0);
}
__global__ void __launch_bounds__(256, 2) k_miller_dbl_var(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e_t, int e, int e_px) {
  VM_KERNEL_PROLOGUE(); vm_miller_dbl_var(w, e_t, e, e_px);
}
__global__ void __launch_bounds__(256, 2) k_miller_sqr_dbl_var(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e_t, int e, int e_px) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  vm_miller_sqr_dbl_var(w, e_t, e, e_px);
}
__global__ void __launch_bounds__(256, 2) k_miller_add_var(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int e_t, int e_b, int which, int e, int e_px) {
  VM_KERNEL_PROLOGUE(); vm_miller_add_var(w, e_t, e_b, which, e, e_px);
}
__global__ void __launch_bounds__(256, 2) k_f12_mul(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int d, int a, int b, int conj_b) {
  __shared__ int32_t park_lds[72 * 256];
  VM_KERNEL_PROLOGUE();
  w.lds = park_lds;
  vm_f12_mul(w, d, a, b, conj_b != 0);
}
// the last product of the final exponentiation with k_g16_compare's work as its tail (bn254_vm.h::vm_f12_mul_eq_const): the other 53 products of a batch stay k_f12_mul
// slot_proof != nullptr (a launch that compacts): status holds the SLOTS' bytes, and every slot that holds a proof hands its final byte to out_status[slot_proof[slot]],
// the caller's buffer in proof order -- the verdict, or what the tail of k_miller_run made of the slot (B outside G2, a deferred error of C, the input count; never 0,
// which is what the slots past the list hold) -- also in a wavefront none of whose proofs is still pending (as k_f12_mul_verdict_keys does for a batch over many keys)
#endif
__global__ void __launch_bounds__(256, 2) k_f12_mul_verdict(int32_t* ws, uint32_t n, uint8_t* status, int d, int a, int b, const int32_t* __restrict__ target, int reject_code,
                                                            const uint32_t* __restrict__ slot_proof, uint8_t* __restrict__ out_status)
#ifdef BN_PLAIN_HALF
{
  __shared__ int32_t park_lds[72 * 256];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint8_t st = status[i < n ? i : n - 1];
  uint8_t out = st;
  if (__builtin_amdgcn_ballot_w64((st & BN254_ST_PENDING) != 0) != 0) {
    DevWs w(ws, n, i < n ? i : DEAD_LANE);
    w.lds = park_lds;
    const bool acc = vm_f12_mul_eq_const(w, d, a, b, target);
    if (st & BN254_ST_PENDING) out = acc ? BN254_ST_ACCEPT : (uint8_t)reject_code;
    if (i < n && (st & BN254_ST_PENDING)) status[i] = out;
  }
  if (slot_proof && i < n && st != 0) out_status[slot_proof[i]] = out;
}
#else
;
#endif
#ifndef BN_PLAIN_HALF
__global__ void __launch_bounds__(256, 2) k_f12_copy(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int d, int a) { VM_KERNEL_PROLOGUE(); vm_f12_copy(w, d, a); }
__global__ void __launch_bounds__(256, 2) k_f12_cyclo_sqr(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int d, int a) { VM_KERNEL_PROLOGUE(); vm_f12_cyclo_sqr(w, d, a); }
__global__ void __launch_bounds__(256, 2) k_f12_cyclo_sqr_n(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int d, int a, int count) {
  VM_KERNEL_PROLOGUE(); vm_f12_cyclo_sqr_n(w, d, a, __builtin_amdgcn_readfirstlane(count));
}
__global__ void __launch_bounds__(256, 2) k_f12_conj(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int d, int a) { VM_KERNEL_PROLOGUE(); vm_f12_conj(w, d, a); }
__global__ void __launch_bounds__(256, 2) k_f12_frob(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int d, int a, int j) { VM_KERNEL_PROLOGUE(); vm_f12_frob(w, d, a, j); }
__global__ void __launch_bounds__(256, 2) k_f12_inv(int32_t* ws, uint32_t n, const uint8_t* __restrict__ status, int d, int a) { VM_KERNEL_PROLOGUE(); vm_f12_inv(w, d, a); }
__global__ void __launch_bounds__(256, 2) k_g16_compare(int32_t* ws, uint32_t n, uint8_t* __restrict__ status, const int32_t* __restrict__ target, int reject_code) {
  VM_KERNEL_PROLOGUE();
  bool acc = vm_f12_eq_const(w, VE_S0, target);
  if (i < n && (st & BN254_ST_PENDING)) status[i] = acc ? BN254_ST_ACCEPT : (uint8_t)reject_code;
}

// =====================================================================================================================
// k_g16_subgroup
// =====================================================================================================================
__global__ void __launch_bounds__(256, 2)
k_g16_subgroup(uint32_t n, int32_t* ws, uint8_t* __restrict__ status, int inputs_match_key, int e_t) {
  // runs AFTER the Miller loop: the r-torsion test of B reads the loop's final G2 point (bn254_vm.h::vm_g2_ate_check)
  VM_KERNEL_PROLOGUE();
  bool ok = vm_g2_ate_check(w, e_t, VE_B);
  if (i < n && (st & BN254_ST_PENDING)) status[i] = g16_subgroup_status(st, ok, inputs_match_key);
}

#endif
}  // namespace bn254
#ifndef BN_PLAIN_HALF

// ---- launch wrappers (C++ linkage, declared in bn254_kernels.h) -----------------------------------------------------------
using namespace bn254;
const char* const bn254_kernel_kind_names[KID_COUNT] = {
  "k_g16_prepare", "k_g16_subgroup", "k_vm_init", "k_f12_sqr", "k_f12_mul_line_fixed",
  "k_f12_mul", "k_f12_cyclo_sqr", "k_f12_conj", "k_f12_frob", "k_f12_inv", "k_g16_compare", "k_f12_copy", "k_f12_cyclo_sqr_n", "k_miller_dbl_var", "k_miller_add_var", "k_g16_msm_partial", "k_g16_msm_reduce", "k_f12_mul_line_fixed2", "k_miller_sqr_dbl_var", "k_miller_step_dbl", "k_miller_step_add", "k_coop12_miller_g16", "k_miller_run"};

// The loader stage of ONE launch, everything before the pairing: the compaction launches, k_g16_prepare, the strict-scalar check and, for a key with many inputs, the
// digit, partial-sum and reduction launches of L.  f says what the caller decided from the launch's form (bn254_g16_plan.h::G16LoaderForm): bn254_launch_g16 fills it
// from g16_launch_form and g16_compacts and leaves the reduction to the rule (g16_wide_reduce8); the value probe bn254_dbg_g16_loader forces each member in turn.
void bn254_launch_g16_loader(const G16LaunchArgs& a, const G16LoaderForm& f, hipStream_t s, G16Prof* prof, G16LoaderRan* ran) {
  G16LoaderRan none;
  G16LoaderRan& r = ran ? *ran : none;      // what is launched, noted where it is launched
  const unsigned grid = grid_for(a.n);
  const uint32_t n = (uint32_t)a.n;
  const bool wide = f.wide, coop = f.coop, compact = f.compact;
  const uint32_t* const slot_proof = compact ? a.slot_proof : nullptr;
  {
    // ONE profile scope, KID_PREPARE: the two launches of the compaction are part of what the loader costs, and the per-kernel profile shows them there
    ProfScope ps_(prof, KID_PREPARE, s);
    if (compact) {
      hipLaunchKernelGGL(k_g16_classify, dim3(grid), dim3(256), 0, s, a.proofs, a.stride, n, a.status, a.block_count);
      hipLaunchKernelGGL(k_g16_compact_write, dim3(grid), dim3(256), 0, s, (const uint8_t*)a.status, n, (const uint32_t*)a.block_count, a.slot_proof, a.slot_status);
      r.compaction = 1;
    }
    hipLaunchKernelGGL(k_g16_prepare, dim3(grid), dim3(256), 0, s, a.proofs, a.stride, a.inputs, a.n_public, n, a.ws, a.status, a.msm_tab, a.k0, a.inputs_match_key, (wide || coop) ? 1 : 0,
                       slot_proof, a.slot_status);
    r.prepare_full = (wide || coop) ? 0 : 1;
  }
  if (a.strict_scalars && a.n_public > 0) { hipLaunchKernelGGL(k_g16_check_scalars, dim3(grid), dim3(256), 0, s, a.inputs, a.n_public, n, a.status); r.check_scalars = 1; }
  if (wide) {
    // inputs of one proof spread over `chunks` lanes, proofs in slices that fit the partial-sum buffer
    const int per = g16_wide_per(knob_wide_per()), chunks = g16_wide_chunks((size_t)a.n_public, per);
    unsigned pg = (unsigned)(((size_t)n * chunks + 255) / 256);
    const bool reduce8 = f.reduce < 0 ? g16_wide_reduce8((size_t)chunks, a.n) : f.reduce == G16_REDUCE_EIGHT;
    {
      ProfScope ps_(prof, KID_MSM_PARTIAL, s);
      if (a.msm_comb) {
        const size_t scalars = (size_t)n * (size_t)a.n_public;
        hipLaunchKernelGGL(k_g16_comb_digits, dim3((unsigned)((scalars + 255) / 256)), dim3(256), 0, s, a.inputs, a.n_public, n, a.msm_digits);
        hipLaunchKernelGGL(k_g16_msm_partial_comb, dim3(pg), dim3(256), 0, s, (const uint16_t*)a.msm_digits, a.n_public, n, per, chunks, (const uint8_t*)a.status, a.msm_tab, a.msm_part);
        r.comb_digits = 1; r.partial = 1;
      }
      else { hipLaunchKernelGGL(k_g16_msm_partial, dim3(pg), dim3(256), 0, s, a.inputs, a.n_public, n, per, chunks, (const uint8_t*)a.status, a.msm_tab, a.msm_part); r.partial = 2; }
      r.chunks = chunks;
    }
    if (reduce8) {
      // eight lanes per proof: below one wavefront per SIMD the reduction is one lane's chain of additions
      ProfScope ps_(prof, KID_MSM_REDUCE, s);
      hipLaunchKernelGGL(k_g16_msm_reduce8, dim3((unsigned)((a.n + 31) / 32)), dim3(256), 0, s, (const int32_t*)a.msm_part, chunks, n, a.ws, a.status, a.k0);
      r.reduce = 2;
    } else {
      BN_LAUNCH(KID_MSM_REDUCE, k_g16_msm_reduce, (const int32_t*)a.msm_part, chunks, n, a.ws, a.status, a.k0);
      r.reduce = 1;
    }
  }
}

hipError_t bn254_launch_g16(const G16LaunchArgs& a, hipStream_t s, hipEvent_t* ev /* 5 events or nullptr */, G16Prof* prof) {
  unsigned grid = grid_for(a.n);
  uint32_t n = (uint32_t)a.n;
  if (ev) (void)hipEventRecord(ev[0], s);
  // the form of this launch -- cooperative kernels (small batches: the public-input MSM moves into the cooperative kernel, twelve lanes per proof, L kept
  // projective, so k_g16_prepare stops after C; keys with many inputs keep their wide MSM kernels and hand L over through the workspace), lane kernels, or
  // their latency mode -- is a pure function of the sizes and the two knobs BN254_COOP and BN254_MILLER_RUN_STEPS (bn254_g16_plan.h), shared with the plan probe
  const G16Form form = g16_launch_form(a.n, (size_t)a.n_public, a.inputs_match_key != 0, a.msm_part != nullptr, a.part_of_larger != 0,
                                       a.split_streams[0] && a.split_streams[1], knob_coop_on(), knob_run_steps_g16());
  const bool wide = form.wide, coop = form.form == G16_FORM_COOP;
  // a launch that compacts (bn254_g16_plan.h): classify, count -> scan -> write, and from k_g16_prepare on every kernel works on the slots of the proofs still pending
  const bool compact = a.slot_proof && a.slot_status && a.block_count && g16_compacts(form, a.key_inputs, a.strict_scalars != 0, a.rlc != 0);
  uint8_t* const lane_status = compact ? a.slot_status : a.status;     // the status bytes the lane kernels read: the slots', or the caller's
  const uint32_t* const slot_proof = compact ? a.slot_proof : nullptr;
  G16LoaderForm lf;
  lf.wide = wide; lf.coop = coop; lf.compact = compact; lf.reduce = G16_REDUCE_RULE;
  bn254_launch_g16_loader(a, lf, s, prof);
  if (ev) (void)hipEventRecord(ev[1], s);
  if (coop) {
    // small batch: cooperative layout (bn254_coop12.hip): public-input MSM, Miller loop of the three pairs, final exponentiation and the verdict in ONE launch
    hipError_t e;
    { ProfScope ps_(prof, KID_COOP_G16, s); e = bn254_coop12_miller_g16(a.ws, a.status, a.n, a.gtab, a.dtab, a.inputs, a.n_public, a.inputs_match_key, a.msm_tab, a.k0, wide ? 1 : 0, a.target, s); }
    if (e != hipSuccess) return e;
    // the r-torsion test of B, the status precedence and the comparison with e(alpha, beta) are the tail of the same launch
    if (ev) { (void)hipEventRecord(ev[2], s); (void)hipEventRecord(ev[3], s); (void)hipEventRecord(ev[4], s); }
    return hipGetLastError();
  }
  LaunchOps ops{a.ws, n, lane_status, grid, s, {a.gtab, a.dtab, nullptr}, prof};
  // The throughput form (the Miller loop as k_miller_run launches) has no k_vm_init, k_g16_subgroup or k_g16_compare: the run that starts at step 0 sets f = 1 and
  // T = (B, 1), the run that ends the loop tests B's subgroup on the point it has just produced and resolves the deferred statuses, and the last product of the final
  // exponentiation compares with e(alpha, beta) -- whichever launches of the plan (88, 44, 22 or 11 steps each) those are.  The latency mode and the one-launch-per-step
  // kernels (BN254_MILLER_RUN_STEPS=0) keep the three kernels.
  const bool folded = form.form == G16_FORM_LANES && form.run_steps > 0;
  if (folded) { ops.run_fold = MR_FOLD_INIT | MR_FOLD_ATE; ops.inputs_match_key = a.inputs_match_key; }
  else BN_LAUNCH(KID_VM_INIT, k_vm_init, a.ws, n, (const uint8_t*)a.status);
  if (form.form == G16_FORM_LATENCY) {
    // latency mode: Miller(A, B) on the launch stream, the two table-driven pairs as their own chains (accumulators in the free
    // slots VE_S1 / VE_S2) on two more streams; f = f_A f_B f_C afterwards.  Three times the squarings, 40 % less time at 4096.
    ops.f12_copy(VE_S1, VE_F); ops.f12_copy(VE_S2, VE_F);
    (void)hipEventRecord(a.split_ev[0], s);
    LaunchOps ob{a.ws, n, a.status, grid, a.split_streams[0], {a.gtab, a.dtab, nullptr}, nullptr};
    LaunchOps oc{a.ws, n, a.status, grid, a.split_streams[1], {a.gtab, a.dtab, nullptr}, nullptr};
    (void)hipStreamWaitEvent(ob.s, a.split_ev[0], 0); (void)hipStreamWaitEvent(oc.s, a.split_ev[0], 0);
    const uint8_t* kinds = miller_step_table().kind;
    for (int st_ = 0; st_ < BN_ATE_STEPS; st_++) {
      const int kind = kinds[st_];
      if (kind == 0) { if (st_ != 0) ops.miller_sqr_dbl_var(VE_T, VE_F, VE_AX); else ops.miller_dbl_var(VE_T, VE_F, VE_AX); }
      else ops.miller_add_var(VE_T, VE_B, kind - 1, VE_F, VE_AX);
      if (kind == 0 && st_ != 0) { ob.f12_sqr(VE_S1); oc.f12_sqr(VE_S2); }
      ob.f12_mul_line_fixed(VE_S1, 0, st_, VE_LX);
      oc.f12_mul_line_fixed(VE_S2, 1, st_, VE_CX);
    }
    (void)hipEventRecord(a.split_ev[1], ob.s); (void)hipEventRecord(a.split_ev[2], oc.s);
    (void)hipStreamWaitEvent(s, a.split_ev[1], 0); (void)hipStreamWaitEvent(s, a.split_ev[2], 0);
    ops.f12_mul(VE_F, VE_F, VE_S1); ops.f12_mul(VE_F, VE_F, VE_S2);
  } else {
    // Steps of the Miller loop per launch (k_miller_run: f never leaves LDS + registers inside a launch).  Large sub-batches take the whole loop in ONE
    // launch; sub-batches that are a single generation of workgroups run measurably better in a few shorter launches (batch 2^17 = two sub-batches of
    // 2^16: 11 steps per launch 5.75 M proofs/s, 22: 5.71, 44: 5.60, 88: 5.49; batch 2^19: 44 best; 2^20: 88 best by 0.7 %; profiles/r03_run_steps_sweep.txt);
    // a batch that is ONE sub-batch (up to 65 536 proofs) takes the whole loop in one launch: 14.23 ms against 14.29 ms with 11 steps at 65 536 (g16_launch_form)
    const int run_steps = form.run_steps;
    if (run_steps) vm_miller_program_runs(ops, run_steps);
    else vm_miller_program(ops, miller_step_table().kind, true);
  }
  if (ev) (void)hipEventRecord(ev[2], s);
  // r-torsion test of B from the loop's final point; resolves the deferred statuses (C errors, input count)
  if (!folded) BN_LAUNCH(KID_SUBGROUP, k_g16_subgroup, n, a.ws, a.status, a.inputs_match_key, (int)VE_T);
  if (ev) (void)hipEventRecord(ev[3], s);
  if (folded) {
    vm_final_exp_program_head(ops);
    BN_LAUNCH(KID_F12_MUL, k_f12_mul_verdict, a.ws, n, lane_status, (int)VE_S0, (int)VE_S2, (int)VE_S0, a.target, BN254_ST_REJECT, slot_proof, a.status);
  } else {
    vm_final_exp_program(ops);
    BN_LAUNCH(KID_COMPARE, k_g16_compare, a.ws, n, a.status, a.target, BN254_ST_REJECT);
  }
  if (ev) (void)hipEventRecord(ev[4], s);
  return hipGetLastError();
}

// ---- a batch over many keys (bn254_keys.h): the lane kernels at every size, the key read per wavefront -------------------------------------------------------
hipError_t bn254_launch_g16_keys(const G16KeysLaunchArgs& a, hipStream_t s) {
  unsigned grid = grid_for(a.m);
  const uint32_t n = (uint32_t)a.m;
  G16Prof* prof = nullptr;
  bn254_launch_g16_prepare_keys(a, grid, s);
  LaunchOps ops{a.ws, n, a.slot_status, grid, s, {nullptr, nullptr, nullptr}, prof};
  ops.key_desc = a.desc; ops.n_keys = a.n_keys; ops.granule_key = a.granule_key;
  // as in bn254_launch_g16: the first run sets f and T, the last one tests B's subgroup (inputs_match from the wavefront's key), the last product compares and scatters
  ops.run_fold = MR_FOLD_INIT | MR_FOLD_ATE;
  // steps per k_miller_run_keys launch: what the single-key lane form takes at this size (g16_launch_form)
  vm_miller_program_runs(ops, g16_launch_form(a.m, 0, true, false, a.part_of_larger != 0, false, false, knob_run_steps_g16_keys()).run_steps);
  vm_final_exp_program_head(ops);
  bn254_launch_f12_mul_verdict_keys(a, grid, s, (int)VE_S0, (int)VE_S2, (int)VE_S0);
  return hipGetLastError();
}

// ---- a SMALL batch over many keys, the direct form: the parse of the records in proof order, then the cooperative kernel that takes the key per proof -------------
hipError_t bn254_launch_g16_keys_direct(const G16KeysDirectArgs& a, hipStream_t s) {
  const uint32_t n = (uint32_t)a.n;
  // wide_msm = 1: the kernel returns after C and never reads the inputs, the tables or K0
  hipLaunchKernelGGL(k_g16_prepare, dim3(grid_for(a.n)), dim3(256), 0, s, a.proofs, a.stride, a.inputs, 0, n, a.ws, a.status, (const int32_t*)nullptr, (const int32_t*)nullptr, 1, 1,
                     (const uint32_t*)nullptr, (uint8_t*)nullptr);
  return bn254_coop12_miller_g16_keys(a.ws, a.status, a.n, a.key_index, a.desc, a.n_keys, a.inputs, a.input_stride, a.strict_scalars, s);
}

// ---- PlonK: the two-fixed-pair pairing check (the MSM stages: bn254_k_msm.hip) -------------------------------------------------------------------
// prod_t e(P_t, Q_t) == 1 for two key-side G2 points (line tables tab0, tab1) and per-item G1 points already in the workspace
// (P_0 at VE_LX, P_1 at VE_CX; identity flags BN254_ST_LINF / BN254_ST_LINF2 in the status byte): ACCEPT or reject_code
hipError_t bn254_launch_pairing2_fixed(int32_t* ws, uint8_t* status, size_t n, const int32_t* tab0, const int32_t* tab1, const int32_t* target_one,
                                       int reject_code, hipStream_t s, hipStream_t aux, hipEvent_t ev_fork, hipEvent_t ev_join) {
  if (knob_coop_on() && n <= knob_coop_fixed_max()) {
    // small batch: the cooperative layout (bn254_coop12.hip), Miller loop of the two pairs, final exponentiation and the comparison in ONE launch
    return bn254_coop12_miller_fixed(ws, status, n, 2, tab0, tab1, target_one, reject_code, s);
  }
  return bn254_launch_pairing2_fixed_lanes(ws, status, n, tab0, tab1, target_one, reject_code, s, aux, ev_fork, ev_join);
}
// the lane form of the check, whatever the size and the knobs say (the device self-test runs it at 64 items: bn254_selftest_dev.hip)
hipError_t bn254_launch_pairing2_fixed_lanes(int32_t* ws, uint8_t* status, size_t n, const int32_t* tab0, const int32_t* tab1, const int32_t* target_one,
                                             int reject_code, hipStream_t s, hipStream_t aux, hipEvent_t ev_fork, hipEvent_t ev_join) {
  unsigned grid = grid_for(n);
  uint32_t nn = (uint32_t)n;
  G16Prof* prof = nullptr;
  LaunchOps ops{ws, nn, status, grid, s, {tab0, tab1, nullptr}, nullptr};
  ops.inf_mask[0] = BN254_ST_LINF; ops.inf_mask[1] = BN254_ST_LINF2;
  BN_LAUNCH(KID_VM_INIT, k_vm_init, ws, nn, (const uint8_t*)status);
  const uint8_t* kinds = miller_step_table().kind;
  if (aux && n <= G16_SPLIT_MAX_PROOFS) {
    // latency mode (as in bn254_launch_g16): the two pairs as two concurrent chains, multiplied at the end
    ops.f12_copy(VE_S1, VE_F);
    (void)hipEventRecord(ev_fork, s);
    LaunchOps ob = ops; ob.s = aux;
    (void)hipStreamWaitEvent(aux, ev_fork, 0);
    for (int st_ = 0; st_ < BN_ATE_STEPS; st_++) {
      if (kinds[st_] == 0 && st_ != 0) { ops.f12_sqr(VE_F); ob.f12_sqr(VE_S1); }
      ops.f12_mul_line_fixed(VE_F, 0, st_, VE_LX);
      ob.f12_mul_line_fixed(VE_S1, 1, st_, VE_CX);
    }
    (void)hipEventRecord(ev_join, aux);
    (void)hipStreamWaitEvent(s, ev_join, 0);
    ops.f12_mul(VE_F, VE_F, VE_S1);
  } else {
    // a large batch (throughput): the whole loop of the two pairs in one launch, the accumulator in flight (k_miller_run_fixed2); BN254_MILLER_RUN_STEPS=0 keeps
    // the one-launch-per-operation form
    const int run_steps = knob_run_steps_pairing2_lanes();
    if (run_steps > 0) {
      for (int s0 = 0; s0 < BN_ATE_STEPS; s0 += run_steps) ops.miller_run_fixed2(s0, s0 + run_steps < BN_ATE_STEPS ? s0 + run_steps : BN_ATE_STEPS, VE_F, VE_LX, VE_CX);
    } else {
      for (int st_ = 0; st_ < BN_ATE_STEPS; st_++) {
        if (kinds[st_] == 0 && st_ != 0) ops.f12_sqr(VE_F);
        ops.f12_mul_line_fixed2(VE_F, st_, VE_LX, VE_CX);
      }
    }
  }
  vm_final_exp_program(ops);
  BN_LAUNCH(KID_COMPARE, k_g16_compare, ws, nn, status, target_one, reject_code);
  return hipGetLastError();
}
hipError_t bn254_launch_pairing2_fixed_keys(int32_t* ws, uint8_t* status, size_t n, const PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key, const int32_t* target_one,
                                            int reject_code, hipStream_t s) {
  unsigned grid = grid_for(n);
  uint32_t nn = (uint32_t)n;
  G16Prof* prof = nullptr;
  LaunchOps ops{ws, nn, status, grid, s, {nullptr, nullptr, nullptr}, nullptr};
  ops.inf_mask[0] = BN254_ST_LINF; ops.inf_mask[1] = BN254_ST_LINF2;
  ops.plonk_desc = desc; ops.n_keys = n_keys; ops.granule_key = granule_key;
  // a pass of up to the knob's slots (bn254_set_plonk_keys_params; BN254_COOP=0: never): the cooperative layout with the key of every item's granule, ONE launch
  if (plonk_keys_coop_form(n))
    return bn254_coop12_miller_fixed_keys(ws, status, n, granule_key, 6, desc, n_keys, target_one, reject_code, s);
  BN_LAUNCH(KID_VM_INIT, k_vm_init, ws, nn, (const uint8_t*)status);
  // steps per launch as in the single-key form (BN254_MILLER_RUN_STEPS; 0 there selects the one-launch-per-operation kernels, which read one key per launch: the whole loop here)
  const int run_steps = knob_run_steps_pairing2_keys();
  for (int s0 = 0; s0 < BN_ATE_STEPS; s0 += run_steps) ops.miller_run_fixed2(s0, s0 + run_steps < BN_ATE_STEPS ? s0 + run_steps : BN_ATE_STEPS, VE_F, VE_LX, VE_CX);
  vm_final_exp_program(ops);
  BN_LAUNCH(KID_COMPARE, k_g16_compare, ws, nn, status, target_one, reject_code);
  return hipGetLastError();
}
// the joint check of a pass with BN254_FLAG_RLC: one "item" per group of 64 slots (k_plonk_group_sums), and group g of a pass is its granule g, so the pass's granule ->
// key words are the key per item.  At most PLONK_MAX_LAUNCH / 64 groups and neighbours of different keys: always the cooperative kernel
hipError_t bn254_launch_pairing2_fixed_groups_keys(int32_t* grp_ws, uint8_t* grp_status, size_t groups, const PlonkKeyDesc* desc, uint32_t n_keys, const uint32_t* granule_key,
                                                   const int32_t* target_one, int reject_code, hipStream_t s) {
  if (groups > bn254_coop_max_proofs_fixed()) return hipErrorInvalidValue;
  return bn254_coop12_miller_fixed_keys(grp_ws, grp_status, groups, granule_key, 0, desc, n_keys, target_one, reject_code, s);
}
#endif
