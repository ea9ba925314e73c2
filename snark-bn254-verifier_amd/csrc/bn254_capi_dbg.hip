// bn254_capi_dbg.hip -- the bn254_dbg_* probes of the C ABI (include/bn254_verify.h; tests and tools): device arithmetic, plans, tables, the
// VALU peak -- and the synthetic workload generator of the bench and the tests.
#include "bn254_capi_internal.h"
#include "bn254_capi_kzg.h"
#include "bn254_kzg.h"
#include <climits>

extern "C" {

int bn254_dbg_key_cache_slots(void) { return KeyCache<bn254_g16_pvk, bn254_groth16_vk_free>::capacity(); }

// Host-only probe of the Groth16 plan (bn254_g16_plan.h): for a key with key_inputs public inputs (comb: its MSM tables are in comb form), a context RESERVED for
// `reserved` proofs and a batch of n proofs with n_public inputs each -- what the context allocates, and every launch the batch makes: out[] receives, per launch,
// 8 values {chunk, first proof of the chunk, proofs, stream slot (-1: caller's stream, not concurrent), form (0 lanes, 1 cooperative, 2 latency mode), Miller steps
// per launch, workspace bytes it addresses (first byte offset, one past the last)}; alloc[] = {workspace bytes, partial-sum bytes, digit bytes, proofs per wide launch}.
// Returns the number of launches through *n_launches (at most max_launches are written).
int bn254_dbg_g16_plan(size_t key_inputs, int comb, size_t reserved, size_t n, size_t n_public, int n_streams, int single_stream, uint64_t alloc[4], uint64_t* out,
                       int max_launches, int* n_launches) {
  if (!alloc || !out || !n_launches || n_streams < 1 || n_streams > 4) return set_err(BN254_E_BAD_ARG, "bad argument");
  const G16Alloc a = g16_alloc_for(reserved, key_inputs, comb != 0);
  alloc[0] = (uint64_t)a.ws_proofs * G16_WS_BYTES_PER_PROOF; alloc[1] = a.msm_part_bytes; alloc[2] = a.msm_digit_bytes; alloc[3] = a.msm_part_proofs;
  int k = 0;
  const size_t chunk = G16_MAX_BATCH;
  int ci = 0;
  for (size_t off = 0; off < n; off += chunk, ci++) {
    const size_t m = n - off < chunk ? n - off : chunk;
    G16ChunkPlan p;
    if (!g16_plan_chunk(p, m, key_inputs, n_public, n_streams, single_stream != 0)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
    for (int pi = 0; pi < p.parts; pi++) {
      const G16Part& q = p.part[pi];
      const G16Form f = g16_launch_form(q.count, n_public, n_public == key_inputs, p.wide, p.parts > 1, p.split_small && p.parts == 1, true, -1);
      if (k < max_launches) {
        uint64_t* o = out + 8 * (size_t)k;
        o[0] = (uint64_t)ci; o[1] = q.first; o[2] = q.count; o[3] = (uint64_t)(int64_t)q.stream_slot; o[4] = (uint64_t)f.form; o[5] = (uint64_t)f.run_steps;
        o[6] = (uint64_t)q.first * G16_WS_BYTES_PER_PROOF; o[7] = (uint64_t)(q.first + q.count) * G16_WS_BYTES_PER_PROOF;
      }
      k++;
    }
  }
  *n_launches = k;
  return BN254_OK;
}

// ... and of the compaction of the lane launches (bn254_g16_plan.h::g16_compacts / g16_compact_alloc): the walk of bn254_dbg_g16_plan for a call with `flags`; per launch
// 6 values {compacts, first slot, slots, first block count, block counts, form}; alloc[] = {slot_proof bytes, slot_status bytes, block count bytes}
int bn254_dbg_g16_compact_plan(size_t key_inputs, size_t reserved, size_t n, size_t n_public, unsigned flags, int n_streams, int single_stream, uint64_t alloc[3],
                               uint64_t* out, int max_launches, int* n_launches) {
  if (!alloc || !out || !n_launches || n_streams < 1 || n_streams > 4) return set_err(BN254_E_BAD_ARG, "bad argument");
  const G16CompactAlloc ca = g16_compact_alloc(g16_alloc_for(reserved, key_inputs, false).ws_proofs, key_inputs);
  alloc[0] = ca.slot_proof_bytes; alloc[1] = ca.slot_status_bytes; alloc[2] = ca.count_bytes;
  int k = 0;
  for (size_t off = 0; off < n; off += G16_MAX_BATCH) {
    const size_t m = n - off < (size_t)G16_MAX_BATCH ? n - off : (size_t)G16_MAX_BATCH;
    G16ChunkPlan p;
    if (!g16_plan_chunk(p, m, key_inputs, n_public, n_streams, single_stream != 0)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
    for (int pi = 0; pi < p.parts; pi++) {
      const G16Part& q = p.part[pi];
      const G16Form f = g16_launch_form(q.count, n_public, n_public == key_inputs, p.wide, p.parts > 1, p.split_small && p.parts == 1, true, -1);
      if (k < max_launches) {
        uint64_t* o = out + 6 * (size_t)k;
        o[0] = g16_compacts(f, key_inputs, (flags & BN254_FLAG_STRICT_SCALARS) != 0, (flags & BN254_FLAG_RLC) != 0) ? 1 : 0;
        o[1] = q.first; o[2] = q.count; o[3] = q.first / G16_COMPACT_BLOCK; o[4] = (q.count + G16_COMPACT_BLOCK - 1) / G16_COMPACT_BLOCK; o[5] = (uint64_t)f.form;
      }
      k++;
    }
  }
  *n_launches = k;
  return BN254_OK;
}
// The launch knobs of the environment as this process read them (bn254_g16_plan.h::launch_knobs, host only): out = {BN254_COOP on, then what BN254_MILLER_RUN_STEPS
// means to bn254_launch_g16, bn254_launch_g16_keys (-1: the plan's choice), bn254_launch_pairing2_fixed_lanes and bn254_launch_pairing2_fixed_keys, then
// BN254_COOP_FIXED_MAX clamped to an int}
int bn254_dbg_launch_knobs(int out[6]) {
  if (!out) return set_err(BN254_E_BAD_ARG, "bad argument");
  const size_t fixed_max = knob_coop_fixed_max();
  out[0] = knob_coop_on() ? 1 : 0;
  out[1] = knob_run_steps_g16(); out[2] = knob_run_steps_g16_keys(); out[3] = knob_run_steps_pairing2_lanes(); out[4] = knob_run_steps_pairing2_keys();
  out[5] = fixed_max > (size_t)INT_MAX ? INT_MAX : (int)fixed_max;
  return BN254_OK;
}
// The count -> scan -> write step on the host: the counts k_g16_classify writes, then for every block what k_g16_compact_write does -- the 256 partial sums of
// g16_compact_partial added up, the block's pending proofs ranked in order, the slots from n' on cleared
int bn254_dbg_g16_compact(const uint8_t* pending, size_t n, unsigned* slot_proof_out, uint8_t* slot_status_out, unsigned* n_pending_out) {
  if (!pending || !slot_proof_out || !slot_status_out || !n_pending_out || n == 0 || n > (size_t)G16_MAX_LAUNCH) return set_err(BN254_E_BAD_ARG, "bad argument");
  const uint32_t blocks = (uint32_t)((n + G16_COMPACT_BLOCK - 1) / G16_COMPACT_BLOCK);
  std::vector<uint32_t> count(blocks, 0);
  for (size_t i = 0; i < n; i++) if (pending[i]) count[i / G16_COMPACT_BLOCK]++;
  for (uint32_t b = 0; b < blocks; b++) {
    uint32_t before = 0, total = 0;
    for (uint32_t t = 0; t < G16_COMPACT_BLOCK; t++) { uint32_t pb, pt; g16_compact_partial(count.data(), blocks, b, t, &pb, &pt); before += pb; total += pt; }
    uint32_t j = before;
    for (uint32_t t = 0; t < G16_COMPACT_BLOCK; t++) {
      const size_t i = (size_t)b * G16_COMPACT_BLOCK + t;
      if (i >= n) break;
      if (pending[i]) { slot_proof_out[j] = (uint32_t)i; slot_status_out[j] = BN254_ST_PENDING; j++; }
      if (i >= total) { slot_proof_out[i] = G16_COMPACT_NO_PROOF; slot_status_out[i] = 0; }
    }
    *n_pending_out = total;
  }
  return BN254_OK;
}

// ... and of the group status bytes of the RLC mode for a chunk of m proofs: what the launch parts address against what a context reserved for `reserved` proofs holds
int bn254_dbg_g16_rlc_plan(size_t reserved, size_t m, int n_streams, int log2_group, int log2_share, size_t min_lanes, uint64_t* need, uint64_t* alloc) {
  if (!need || !alloc || m == 0 || n_streams < 1 || n_streams > 4 || log2_group < 1 || log2_group > 16 || log2_share < 0 || log2_share > 3) return set_err(BN254_E_BAD_ARG, "bad argument");
  G16RlcChunkPlan p;
  if (!g16_plan_rlc_chunk(p, m, n_streams, log2_group, log2_share, min_lanes)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
  *need = p.need; *alloc = g16_rlc_alloc(reserved);
  return BN254_OK;
}

// ... and of the wide form (keys with more than RLC_MAX_PUBLIC inputs): alloc = {row, digit, partial-sum bytes} rlc_ensure allocates for a chunk of m proofs;
// parts_out: 2 values per launch part {first group, groups} as g16_enqueue_rlc places them (at most max_parts written, *n_parts = parts)
int bn254_dbg_g16_rlc_wide_plan(size_t m, int n_streams, int log2_group, int log2_share, size_t min_lanes, size_t key_inputs, int msm_form, uint64_t alloc[3],
                                uint64_t* parts_out, int max_parts, int* n_parts) {
  if (!alloc || !n_parts || m == 0 || m > (size_t)G16_MAX_BATCH || n_streams < 1 || n_streams > 4 || log2_group < 1 || log2_group > 16 || log2_share < 0 || log2_share > 3 ||
      msm_form < 0 || msm_form > 2 || (max_parts > 0 && !parts_out))
    return set_err(BN254_E_BAD_ARG, "bad argument");
  G16RlcChunkPlan p;
  if (!g16_plan_rlc_chunk(p, m, n_streams, log2_group, log2_share, min_lanes)) return set_err(BN254_E_BAD_ARG, "batch cannot be planned");
  const G16RlcWide a = g16_rlc_wide_alloc(g16_round256(p.wide_groups), key_inputs, msm_form);
  alloc[0] = a.rows_bytes; alloc[1] = a.digit_bytes; alloc[2] = a.part_bytes;
  for (int k = 0; k < p.parts && k < max_parts; k++) { parts_out[2 * k] = p.part[k].wide_off; parts_out[2 * k + 1] = p.part[k].plan.groups; }
  *n_parts = p.parts;
  return BN254_OK;
}

// The stream-overlap decision (bn254_overlap_vote.h) replayed over the batches of one (key, device), without a device: the functions g16_enqueue_exact calls, in its
// order, every recorded measurement there to be read by the next batch (arguments: include/bn254_verify.h)
int bn254_dbg_overlap_replay(const uint8_t* kind, const float* timings, size_t n_batches, int fallback, int* out, float* ratio_out) {
  if (n_batches && (!kind || !timings || !out || !ratio_out)) return set_err(BN254_E_BAD_ARG, "bad argument");
  OvVote v;
  size_t recorded = 0;   // the batch whose events are waiting to be read
  for (size_t b = 0; b < n_batches; b++) {
    if (kind[b] > 2) return set_err(BN254_E_BAD_ARG, "bad argument");
    if (v.state == 1) {
      const float* t = timings + 4 * recorded;
      const float ratio = ov_ratio(t[0], t[1], t[2], t[3]);
      ov_read(v, kind[recorded] == 1 ? &ratio : nullptr, fallback != 0);
    }
    const bool probe_now = ov_begin_batch(v), single_stream = v.single_stream && !probe_now;
    if (ov_measures(v, kind[b] != 0 && !single_stream, 2, 1, 1)) { v.state = 1; recorded = b; }
    int* o = out + 4 * b;
    o[0] = probe_now; o[1] = single_stream; o[2] = v.state; o[3] = v.serial_votes;
    ratio_out[b] = v.ratio;
  }
  return BN254_OK;
}

// Host compile of the wide RLC group stage (bn254_rlc.h): the group scalars s_gj = sum r_i x_ij of every group of rlc_plan(n, log2_group, log2_share) from
// given weights (16 bytes per proof: k1, k2 as little-endian u64; r_i = k1 + k2 lambda) and liveness bytes (0: weight 0), and for group `group` the
// point L = t_0 K_0 + sum_j s_j K_j through vm_rlc_group_points_wide with 13-bit window entries of the key points (computed on the fly).  kpts: K_0 .. K_n_public,
// 64-byte uncompressed each.  scalars_out (groups x n_public x 32 bytes, big-endian; nullptr: only *groups_out) ; l_out: L uncompressed, all zero for the identity.
namespace {
struct HostLane {
  Fp e[VE_COUNT];
  Fp ld(int i) const { return e[i]; }
  void st(int i, const Fp& a) { e[i] = a; }
};
struct LazyWindows {   // entry d of window w of P: (d + 1) 2^(MSM_FW_BITS w) P, affine
  std::vector<G1Proj> bw;
  explicit LazyWindows(const G1Aff& P) : bw(MSM_FW_WINDOWS) {
    G1Proj b = g1_from_affine(P);
    for (int w = 0; w < MSM_FW_WINDOWS; w++) { bw[w] = b; for (int k = 0; k < MSM_FW_BITS; k++) b = g1_dbl(b); }
  }
  G1Aff operator()(int w, int d) const {
    const uint32_t m = (uint32_t)d + 1;
    G1Proj acc = g1_identity();
    for (int bit = MSM_FW_BITS - 1; bit >= 0; bit--) { acc = g1_dbl(acc); if ((m >> bit) & 1) acc = g1_add(acc, bw[w]); }
    return g1_to_affine(acc);
  }
};
}  // namespace
// BN254_FLAG_COMPRESSED_PROOFS: the body of k_g16_decompress (bn254_codec.h), compiled for the host, over k records
int bn254_dbg_g16_decompress(const uint8_t* records, size_t stride, size_t k, uint8_t* raw_out, uint8_t* pre_out) {
  if ((k && (!records || !raw_out || !pre_out)) || stride < 128) return set_err(BN254_E_BAD_ARG, "bad argument");
  for (size_t i = 0; i < k; i++) {
    uint32_t in[32], out[64];
    memcpy(in, records + i * stride, 128);
    pre_out[i] = g16_decompress_record(in, out) ? 0 : 1;
    memcpy(raw_out + i * 256, out, 256);
  }
  return BN254_OK;
}
int bn254_dbg_rlc_wide_group(const uint8_t* kpts, const uint8_t alpha64[64], const uint8_t* weights, const uint8_t* live, const uint8_t* inputs, size_t n_public, size_t n,
                             int log2_group, int log2_share, unsigned group, uint8_t* scalars_out, unsigned* groups_out, uint8_t l_out[64]) {
  if (!groups_out || n == 0 || n > (size_t)G16_MAX_LAUNCH || log2_group < 1 || log2_group > 16 || log2_share < 0 || log2_share > log2_group || log2_share > 3 || (n >> log2_share) == 0)
    return set_err(BN254_E_BAD_ARG, "bad argument");
  const RlcPlan plan = rlc_plan((uint32_t)n, log2_group, log2_share);
  *groups_out = plan.groups;
  if (!scalars_out) return BN254_OK;
  if (!kpts || !alpha64 || !weights || !live || (n_public && !inputs) || !l_out || group >= plan.groups) return set_err(BN254_E_BAD_ARG, "bad argument");
  auto load_input = [&](uint32_t i, int j, uint32_t x[8]) { words_from_be(x, inputs + ((size_t)i * n_public + (size_t)j) * 32); };
  auto load_weight = [&](uint32_t i, uint32_t k[4]) -> bool {
    if (!live[i]) return false;
    for (int q = 0; q < 4; q++) { const uint8_t* b = weights + 16 * (size_t)i + 4 * q; k[q] = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }
    return true;
  };
  for (uint32_t g = 0; g < plan.groups; g++)
    for (size_t j = 0; j < n_public; j++) {
      const Fr8 sj = rlc_group_scalar(g, (int)j, (uint32_t)n, plan, load_input, load_weight);
      words_to_be(scalars_out + ((size_t)g * n_public + j) * 32, sj.w);
    }
  // the group's lane after the fold: t_0 = sum of its live weights, C' = O
  Fr8 t0 = fr8_zero();
  rlc_for_each_member(group, (uint32_t)n, plan, [&](uint32_t i) { uint32_t k[4]; if (load_weight(i, k)) t0 = fr8_add(t0, rlc_weight(k)); });
  HostLane w;
  for (auto& e : w.e) e = fp_zero();
  w.st(RLC_T, fr8_to_slot(t0));
  w.st(RLC_C, fp_zero()); w.st(RLC_C + 1, fp_one()); w.st(RLC_C + 2, fp_zero());
  std::vector<LazyWindows> kw;
  for (size_t j = 0; j <= n_public; j++) {
    G1Aff K; K.x = fp_from_be(kpts + 64 * j); K.y = fp_from_be(kpts + 64 * j + 32);
    if (!g1_on_curve(K)) return set_err(BN254_E_BAD_ARG, "key point not on the curve");
    kw.emplace_back(K);
  }
  G1Aff A; A.x = fp_from_be(alpha64); A.y = fp_from_be(alpha64 + 32);
  if (!g1_on_curve(A)) return set_err(BN254_E_BAD_ARG, "alpha not on the curve");
  const LazyWindows na(g1_neg(A));
  G1Proj Lk = g1_identity();
  for (size_t j = 0; j < n_public; j++) {
    Fr8 sj;
    words_from_be(sj.w, scalars_out + ((size_t)group * n_public + j) * 32);
    Lk = g1_window_sum(Lk, sj, [&](int wi, int d) { return kw[j + 1](wi, d); });
  }
  const int fl = vm_rlc_group_points_wide(w, Lk, [&](int b, int wi, int d) { return b == 0 ? na(wi, d) : kw[0](wi, d); });
  if (fl & 1) { memset(l_out, 0, 64); return BN254_OK; }
  G1Aff L; L.x = w.ld(VE_LX); L.y = w.ld(VE_LY);
  enc_g1_uncompressed(l_out, L);
  return BN254_OK;
}

// The host image of a prepared Groth16 key, for the tests that hold two handles of the same key against each other (bn254_groth16_vk_prepare_batch against
// bn254_groth16_vk_prepare): dwords n_k (2) | msm_comb | then k0, gtab, dtab, target, kpts, each as its length and its dwords | alpha (18), k0_pt (18), b_arg (36) as
// canonical digits.  *len: the bytes the image takes (written whenever the pointer is given); out may be null or too small (cap): BN254_E_BAD_ARG then.
int bn254_dbg_g16_pvk_image(const bn254_g16_pvk* pvk, uint8_t* out, size_t cap, size_t* len) {
  if (!pvk || !len) return set_err(BN254_E_BAD_ARG, "bad argument");
  const G16Prepared& h = pvk->host;
  std::vector<int32_t> im;
  im.push_back((int32_t)(uint32_t)h.n_k); im.push_back((int32_t)(uint32_t)((uint64_t)h.n_k >> 32)); im.push_back(h.msm_comb ? 1 : 0);
  for (const std::vector<int32_t>* v : {&h.k0, &h.gtab, &h.dtab, &h.target, &h.kpts}) { im.push_back((int32_t)v->size()); im.insert(im.end(), v->begin(), v->end()); }
  int32_t d[2 * BN_NL];
  fp_to_limbs(d, h.alpha.x); fp_to_limbs(d + BN_NL, h.alpha.y); im.insert(im.end(), d, d + 2 * BN_NL);
  fp_to_limbs(d, h.k0_pt.x); fp_to_limbs(d + BN_NL, h.k0_pt.y); im.insert(im.end(), d, d + 2 * BN_NL);
  put_fp2(d, h.b_arg.x); im.insert(im.end(), d, d + 2 * BN_NL);
  put_fp2(d, h.b_arg.y); im.insert(im.end(), d, d + 2 * BN_NL);
  *len = im.size() * 4;
  if (!out || cap < *len) return set_err(BN254_E_BAD_ARG, "image buffer too small");
  memcpy(out, im.data(), *len);
  return BN254_OK;
}
// bn254_groth16_vk_prepare_batch with a choice of where the kernels' bodies run: device -1 is their host compile (csrc/bn254_vkprep.h; no device is touched), a device
// ordinal the kernels.  stage_ms: null, or 5 floats -- G1 decode, G2 decode, fold, line tables, pairing, summed over the passes, from HIP events (zero on the host).
// (bn254_capi_vkbatch.hip is not part of the one-translation-unit host build: a harness that includes it defines BN254_HOSTSAN_VKBATCH.)
#if defined(__HIPCC__) || defined(BN254_HOSTSAN_VKBATCH)
int bn254_dbg_g16_vk_prepare_batch(const uint8_t* const* vks, const size_t* vk_lens, size_t n_keys, unsigned mode, int device, bn254_g16_pvk** out, int* key_status,
                                   float* stage_ms) {
  if (device < -1) return set_err(BN254_E_BAD_ARG, "bad argument");
  return vkp_prepare_batch(vks, vk_lens, n_keys, mode, device == -1, device, out, key_status, stage_ms);
}
#endif

// ---------------------------------------------------------------- device-arithmetic probes (tests)
static int run_probe(size_t in_a, size_t in_b, size_t out_sz, const uint8_t* a, const uint8_t* b, uint8_t* o, size_t n, int device,
                     hipError_t (*launch)(const uint8_t*, const uint8_t*, uint8_t*, size_t)) {
  int rc = check_device(device);
  if (rc) return rc;
  if (n == 0) return BN254_OK;
  DevBuf<uint8_t> da, db, dout;   // released on every exit path
  if ((rc = da.ensure(in_a * n))) return rc;
  HIPCK(hipMemcpy(da, a, in_a * n, hipMemcpyHostToDevice));
  if (in_b && b) { if ((rc = db.ensure(in_b * n))) return rc; HIPCK(hipMemcpy(db, b, in_b * n, hipMemcpyHostToDevice)); }
  if ((rc = dout.ensure(out_sz * n))) return rc;
  hipError_t e = launch(da, db, dout, n);
  if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("probe launch: ") + hipGetErrorString(e));
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(o, dout, out_sz * n, hipMemcpyDeviceToHost));
  return BN254_OK;
}
// probe (tests): stage 1 of the device path alone -- zeta (32-byte big-endian, canonical; zero where the proof failed before the challenges) and the
// stage-1 status of each proof (BN254_ACCEPT = alive, or the error code the stage decided)
int bn254_dbg_plonk_stage1(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n,
                           uint8_t* zeta_out, uint8_t* status_out, int device) {
  if (!pvk || !proofs || !zeta_out || !status_out || n == 0 || n > PLONK_MAX_LAUNCH) return set_err(BN254_E_BAD_ARG, "bad argument");
  PlonkDev* d;
  int rc;
  {
    std::lock_guard<std::mutex> lk(pvk->mu);
    if ((rc = plonk_ensure_dev(pvk, device, &d))) return rc;
  }
  PlonkLease lease(d, 1);
  PlonkCtx& c = lease.ctx(0);
  if ((rc = plonk_ensure_ctx(pvk, c, n, 0))) return rc;
  const size_t pb = n * proof_stride, ib = n * n_public * 32;
  DevBuf<uint8_t> in, zo, so;
  if ((rc = in.ensure(pb + ib + 4)) || (rc = zo.ensure(32 * n)) || (rc = so.ensure(n))) return rc;
  HIPCK(hipMemcpy(in, proofs, pb, hipMemcpyHostToDevice));
  if (ib) HIPCK(hipMemcpy(in + pb, public_inputs, ib, hipMemcpyHostToDevice));
  uint32_t lam_key[11] = {0};
  hipError_t e = bn254_launch_plonk_stage1(d->d_key, in, proof_stride, in + pb, n_public, n, lam_key, c.d_work, c.terms, c.flags, plonk_stage1_terms(pvk->key), c.stream);
  if (e == hipSuccess) e = bn254_launch_plonk_dbg_zeta(c.d_work, n, zo, so, c.stream);
  if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("probe launch: ") + hipGetErrorString(e));
  HIPCK(hipStreamSynchronize(c.stream));
  HIPCK(hipMemcpy(zeta_out, zo, 32 * n, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(status_out, so, n, hipMemcpyDeviceToHost));
  return BN254_OK;
}

// ---------------------------------------------------------------- value-level probes of the PlonK stages (tests/test_gpu_plonk_stage_values.py)
// The product's own pass up to the pairing operands (plonk_pass_points: stage 1 -> digest MSM -> stage 2 -> KZG MSM) under a ChaCha20 key the CALLER gives, and what it
// left for every proof, in proof order, as records of PLS_REC bytes (include/bn254_verify.h has the layout).  The public entries cannot be handed a key: they draw
// theirs inside plonk_pass.
namespace {
enum { PLS_REC = 560, PLS_MAX_PROOFS = 4096, PLS_O_P0 = 432, PLS_O_P1 = 496 };
// the record of one proof from what the device (or the host compile) left: dev = the PLONK_DBG_STAGES_DEV_BYTES of k_plonk_dbg_stages, p0 / p1 = the affine points as
// stored at VE_LX / VE_CX (read only while the proof is pending)
void pls_record(uint8_t* rec, const uint8_t* dev, const uint8_t* p0, const uint8_t* p1, uint32_t slot) {
  memset(rec, 0, PLS_REC);
  memcpy(rec, dev, PLONK_DBG_STAGES_DEV_BYTES);
  const uint8_t st = dev[1];
  for (int k = 0; k < 4; k++) rec[8 + k] = (uint8_t)(slot >> (8 * k));
  if (!(st & BN254_ST_PENDING)) return;       // decided: the byte is the proof's status, and no point of it was stored
  rec[1] = (st & 0x1f) ? (uint8_t)(st & 0x1f) : (uint8_t)BN254_ACCEPT;
  rec[3] = (st & BN254_ST_LINF) ? 1 : 0; rec[4] = (st & BN254_ST_LINF2) ? 1 : 0;
  if (!rec[3]) memcpy(rec + PLS_O_P0, p0, 64);
  if (!rec[4]) memcpy(rec + PLS_O_P1, p1, 64);
}
// sum s of a launch's shape over the terms a stage wrote for one proof, term by term with the host's G1 arithmetic: no plan, no rows, no window tables
G1Proj pls_host_sum(const PlonkKey& key, const MsmShape& sh, int s, const MsmTerm* t, const uint8_t* fl) {
  auto mul = [](const G1Aff& P, const uint32_t* w, int nw) {
    G1Proj acc = g1_identity();
    const G1Proj b = g1_from_affine(P);
    for (int bit = 32 * nw - 1; bit >= 0; bit--) { acc = g1_dbl(acc); if ((w[bit >> 5] >> (bit & 31)) & 1u) acc = g1_add(acc, b); }
    return acc;
  };
  auto point = [](const MsmTerm& e) { G1Aff P; P.x = fp_from_limbs(e.pt); P.y = fp_from_limbs(e.pt + BN_NL); return P; };
  G1Proj L = g1_identity();
  for (int i = 0; i < sh.n_var[s]; i++) {            // (+-k1 +- k2 lambda) P, the halves and signs as put_term left them; flag bit 0: P is the identity
    const int q = sh.var_term[s][i];
    if (fl[q] & 1) continue;
    const G1Aff P = point(t[q]);
    G1Aff P2; P2.x = fp_mul(P.x, fp_from_limbs(BN_GLV_BETA)); P2.y = P.y;
    L = g1_add(L, mul((fl[q] & 2) ? g1_neg(P) : P, t[q].k, 4));
    L = g1_add(L, mul((fl[q] & 4) ? g1_neg(P2) : P2, t[q].k + 4, 4));
  }
  for (int i = 0; i < sh.n_unit[s]; i++) {
    const int q = sh.unit_term[s][i];
    if (fl[q] & 1) continue;
    const G1Aff P = point(t[q]);
    L = g1_add(L, g1_from_affine((fl[q] & 2) ? g1_neg(P) : P));
  }
  for (int i = 0; i < sh.n_fixed[s]; i++) L = g1_add(L, mul(plonk_table_point(key, sh.fixed_tab[s][i]), t[sh.fixed_term[s][i]].k, 8));
  return L;
}
// The host compile of the same stage source, proof by proof: plonk_stage1, lambda and the weight derived as bn254_plonk_self_test restates them, plonk_stage2, and each
// sum added up by pls_host_sum.  No device is touched
int pls_on_host(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n, const uint32_t lam_key[11],
                bool weighted, uint8_t* out) {
  const PlonkKey& key = pvk->key;
  const FrCtx& F = fr_ctx();
  const int T1 = plonk_stage1_terms(key), T2 = plonk_stage2_terms(key), TT = T2 + 2;
  bn254::ChaChaKey lk, wk_;
  for (int i = 0; i < 8; i++) lk.k[i] = lam_key[i];
  for (int i = 0; i < 3; i++) lk.nonce[i] = lam_key[8 + i];
  wk_ = lk; wk_.nonce[2] ^= 0x00524c43u;
  std::vector<MsmTerm> t1((size_t)T1), t2((size_t)TT); std::vector<uint8_t> f1((size_t)T1), f2((size_t)TT);
  auto put_point = [](uint8_t* o, const G1Proj& L) { if (!g1_is_identity(L)) enc_g1_uncompressed(o, g1_to_affine(L)); };
  for (size_t i = 0; i < n; i++) {
    uint8_t dev[PLONK_DBG_STAGES_DEV_BYTES], p0[64], p1[64];
    memset(dev, 0, sizeof dev); memset(p0, 0, 64); memset(p1, 0, 64);
    const uint8_t* proof = proofs + i * proof_stride;
    PlonkWork wk; memset((void*)&wk, 0, sizeof wk);
    memset((void*)t1.data(), 0, t1.size() * sizeof(MsmTerm)); memset(f1.data(), 0, f1.size());
    const int st = plonk_stage1(key, proof, proof_stride, public_inputs + i * n_public * 32, n_public, wk, t1.data(), f1.data());
    dev[0] = dev[1] = (uint8_t)st;
    if (st == PL_OK || st == PL_OPENING) F.to_be(dev + 16, wk.zeta);
    if (st == PL_OK) {
      uint32_t lw[12]; for (int j = 0; j < 3; j++) bn254::chacha20_block4(lw + 4 * j, lk, 3u * (uint32_t)i + (uint32_t)j);
      uint8_t lb[48]; for (int j = 0; j < 12; j++) { lb[4 * j] = (uint8_t)lw[j]; lb[4 * j + 1] = (uint8_t)(lw[j] >> 8); lb[4 * j + 2] = (uint8_t)(lw[j] >> 16); lb[4 * j + 3] = (uint8_t)(lw[j] >> 24); }
      wk.lambda = F.from_be_reduce(lb, 48);
      F.to_be(dev + 48, wk.lambda); F.to_be(dev + 80, wk.lin_opening);
      for (uint32_t k = 0; k < key.n_qcp; k++) F.to_be(dev + 176 + 32 * k, bsb22_hash_to_field(proof + wk.pr.off_bsb + 64 * (size_t)k));
      const G1Proj lin = pls_host_sum(key, pvk->shape1, 0, t1.data(), f1.data());
      const bool lin_inf = g1_is_identity(lin);
      uint32_t lin_words[16] = {0};
      if (lin_inf) dev[2] = 1;
      else { const G1Aff a = g1_to_affine(lin); fp_to_words(lin_words, a.x); fp_to_words(lin_words + 8, a.y); enc_g1_uncompressed(dev + 112, a); }
      FrM wgt = {{0, 0, 0, 0}};
      if (weighted) {
        uint32_t rw[4]; bn254::chacha20_block4(rw, wk_, (uint32_t)i);
        uint8_t rb[16];
        rw[0] |= 1u;
        for (int j = 0; j < 4; j++) { rb[15 - 4 * j] = (uint8_t)rw[j]; rb[14 - 4 * j] = (uint8_t)(rw[j] >> 8); rb[13 - 4 * j] = (uint8_t)(rw[j] >> 16); rb[12 - 4 * j] = (uint8_t)(rw[j] >> 24); }
        wgt = F.from_be_reduce(rb, 16);
      }
      wk.pr.raw = proof;
      plonk_stage2(key, proof, wk, lin_words, lin_inf, t2.data(), f2.data(), t2.data() + T2, weighted ? &wgt : nullptr);
      const MsmShape& sh2 = weighted ? pvk->shape2_rlc : pvk->shape2;
      const G1Proj P0 = pls_host_sum(key, sh2, 0, t2.data(), f2.data()), P1 = pls_host_sum(key, sh2, 1, t2.data(), f2.data());
      dev[1] = (uint8_t)(BN254_ST_PENDING | (g1_is_identity(P0) ? BN254_ST_LINF : 0) | (g1_is_identity(P1) ? BN254_ST_LINF2 : 0));
      put_point(p0, P0); put_point(p1, P1);
    }
    pls_record(out + i * PLS_REC, dev, p0, p1, (uint32_t)i);
  }
  return BN254_OK;
}
#if defined(__HIPCC__)
// what a pass of m proofs (slots) left on context c -> the device halves of the records and the stored points, on the host.  Enqueued behind the pass on c.stream
int pls_fetch(PlonkCtx& c, size_t m, uint32_t n_h2f, std::vector<uint8_t>& dev, std::vector<uint8_t>& pts) {
  int rc;
  DevBuf<uint8_t> d_dev, d_pts;
  if ((rc = d_dev.ensure(m * (size_t)PLONK_DBG_STAGES_DEV_BYTES)) || (rc = d_pts.ensure(384 * m))) return rc;
  hipError_t e = bn254_launch_plonk_dbg_stages(c.d_work, c.words, c.inf, c.status, m, n_h2f, d_dev, c.stream);
  // elements 6 .. 17 as one Fp12 in the store's byte order: (VE_CX, VE_CY) first, (VE_LX, VE_LY) fourth (as bn254_dbg_g1_msm reads them in out_mode 1)
  if (e == hipSuccess) e = bn254_launch_dbg_store(c.ws, m, (int)VE_CX_ELEM, d_pts, 0, c.stream);
  if (e != hipSuccess) return launch_err(e, "probe");
  HIPCK(hipStreamSynchronize(c.stream));
  dev.resize(m * (size_t)PLONK_DBG_STAGES_DEV_BYTES); pts.resize(384 * m);
  HIPCK(hipMemcpy(dev.data(), d_dev, dev.size(), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(pts.data(), d_pts, pts.size(), hipMemcpyDeviceToHost));
  return BN254_OK;
}
int pls_on_device(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n, const uint32_t lam_key[11],
                  bool weighted, uint8_t* out, int device) {
  PlonkDev* d;
  int rc;
  {
    std::lock_guard<std::mutex> lk(pvk->mu);
    if ((rc = plonk_ensure_dev(pvk, device, &d))) return rc;
  }
  PlonkLease lease(d, 1);
  PlonkCtx& c = lease.ctx(0);
  if ((rc = plonk_ensure_ctx(pvk, c, n, 0))) return rc;
  const size_t pb = n * proof_stride, ib = n * n_public * 32;
  DevBuf<uint8_t> in;
  if ((rc = in.ensure(pb + ib + 4))) return rc;
  HIPCK(hipMemcpy(in, proofs, pb, hipMemcpyHostToDevice));
  if (ib) HIPCK(hipMemcpy(in + pb, public_inputs, ib, hipMemcpyHostToDevice));
  // the arguments of plonk_run_device: records and rows back to back, as the host-buffer entry stages them
  std::vector<uint8_t> dev, pts;
  rc = plonk_pass_points(pvk, PlonkTables{d, nullptr, 0, nullptr, d->one}, PlonkPassIn{in, proof_stride, in + pb, n_public, 0, 0, 0}, c, n, lam_key, weighted, nullptr);
  if (!rc) rc = pls_fetch(c, n, pvk->key.n_qcp, dev, pts);
  if (rc) { const std::string keep = g_err; (void)hipStreamSynchronize(c.stream); return set_err(rc, keep); }
  for (size_t i = 0; i < n; i++) pls_record(out + i * PLS_REC, dev.data() + i * PLONK_DBG_STAGES_DEV_BYTES, pts.data() + 384 * i + 192, pts.data() + 384 * i, (uint32_t)i);
  return BN254_OK;
}
#endif
}  // namespace
static_assert(PLONK_DBG_STAGES_DEV_BYTES == PLS_O_P0, "the device half of a probe record ends where the points begin");

int bn254_dbg_plonk_stages(const bn254_plonk_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n,
                           const unsigned lam_key[11], unsigned flags, uint8_t* out, int device) {
  int rc = check_batch_args(true, pvk, proofs, proof_stride, public_inputs, n_public, n, out, flags);
  if (rc) return rc;
  if (!lam_key || !out || !proofs || n == 0 || n > (size_t)PLS_MAX_PROOFS || device < -1) return set_err(BN254_E_BAD_ARG, "bad argument: 1 .. 4096 proofs, a key of 11 words, device -1 (host) or an ordinal");
  const bool weighted = (flags & BN254_FLAG_RLC) != 0;
  if (device < 0) return pls_on_host(pvk, proofs, proof_stride, public_inputs, n_public, n, lam_key, weighted, out);
#if defined(__HIPCC__)
  return pls_on_device(pvk, proofs, proof_stride, public_inputs, n_public, n, lam_key, weighted, out, device);
#else
  return set_err(BN254_E_NO_DEVICE, "the device half of the probe is not part of a host build");
#endif
}
#if defined(__HIPCC__)
int bn254_dbg_plonk_stages_keys(const bn254_plonk_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride,
                                const uint8_t* public_inputs, size_t input_stride, size_t n, const unsigned lam_key[11], unsigned flags, uint8_t* out, int device) {
  if (!lam_key || !out || n == 0 || n > (size_t)PLS_MAX_PROOFS || device < 0) return set_err(BN254_E_BAD_ARG, "bad argument: 1 .. 4096 proofs, a key of 11 words, a device ordinal");
  const bool weighted = (flags & BN254_FLAG_RLC) != 0;
  return plonk_keys_probe_pass(pvks, n_keys, key_index, proofs, proof_stride, public_inputs, input_stride, n, flags, device, [&](const PlonkKeysProbePass& p) -> int {
    int rc = plonk_pass_points(p.shapes, p.t, p.in, *p.c, p.slots, lam_key, weighted, nullptr);
    std::vector<uint8_t> dev, pts;
    if (rc || (rc = pls_fetch(*p.c, p.slots, p.shapes->key.n_qcp, dev, pts))) return rc;
    std::vector<uint32_t> s2p(p.slots);
    HIPCK(hipMemcpy(s2p.data(), p.slot_to_proof, p.slots * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint8_t> seen(n, 0);
    for (size_t j = 0; j < p.slots; j++) {
      const uint32_t i = s2p[j];
      if (i >= n) continue;                                 // a padding slot
      if (seen[i]) return set_err(BN254_E_HIP, "grouping gave a proof two slots");
      seen[i] = 1;
      pls_record(out + (size_t)i * PLS_REC, dev.data() + j * PLONK_DBG_STAGES_DEV_BYTES, pts.data() + 384 * j + 192, pts.data() + 384 * j, (uint32_t)j);
    }
    for (size_t i = 0; i < n; i++) if (!seen[i]) return set_err(BN254_E_HIP, "grouping left a proof without a slot");
    return BN254_OK;
  });
}
#endif

// the multiply-add issue rate of THIS device (lane-level v_mad_u64_u32 per second, sixteen independent chains per lane, four wavefronts per SIMD, best of five
// launches of ~0.25 ms): what bench.py divides its VALU rooflines by (the constant of profiles/r01_ubench_valu.txt, 35.1e12, stays as the reference)
int bn254_dbg_valu_peak(int device, double* mads_per_s) {
  if (!mads_per_s) return set_err(BN254_E_BAD_ARG, "bad argument");
  int rc = check_device(device);
  if (rc) return rc;
  *mads_per_s = bn254_measure_valu_peak(12);
  return *mads_per_s > 0 ? BN254_OK : set_err(BN254_E_HIP, "peak measurement failed");
}
int bn254_dbg_valu_peak_sustained(int device, double ms_target, double* mads_per_s) {
  if (!mads_per_s || !(ms_target > 0.0) || ms_target > 2000.0) return set_err(BN254_E_BAD_ARG, "bad argument");
  int rc = check_device(device);
  if (rc) return rc;
  *mads_per_s = bn254_measure_valu_sustained(ms_target);
  return *mads_per_s > 0 ? BN254_OK : set_err(BN254_E_HIP, "peak measurement failed");
}
int bn254_dbg_fp_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int device) {
  return run_probe(32, 32, 32, a, b, out, n, device, [](const uint8_t* x, const uint8_t* y, uint8_t* o, size_t m) { return bn254_launch_dbg_fp_mul(x, y, o, m, nullptr); });
}
static thread_local int g_probe_op = 0;
static thread_local DevBuf<int32_t> g_probe_ws;      // held for the duration of one probe call: the launchers below are captureless lambdas
static thread_local DevBuf<uint8_t> g_probe_kinds;
static int probe_ws_alloc(size_t n, int device) {
  int rc = check_device(device);
  if (rc) return rc;
  if (n > G16_MAX_LAUNCH) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  if ((rc = g_probe_ws.ensure((n ? n : 1) * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = g_probe_kinds.ensure(n ? n : 1))) { g_probe_ws.release(); return rc; }  // kinds: status bytes of the probe lanes
  return BN254_OK;
}
static void probe_ws_free() { g_probe_ws.release(); g_probe_kinds.release(); }
// Fp12 operands and results of the value-level probes: format 0 = 384 bytes, 1 = 108 raw int32 digits per value (include/bn254_verify.h)
static inline size_t probe_fmt_bytes(int format) { return format ? (size_t)12 * BN_NL * sizeof(int32_t) : (size_t)384; }
static thread_local int g_probe_in = 0, g_probe_out = 0;
int bn254_dbg_fp12_op_fmt(int op, const void* a, const void* b, void* out, size_t n, int in_format, int out_format, int device) {
  const bool two = op == 0 || op == 8 || op == 9;
  if (op < 0 || op > 9 || (in_format | out_format) & ~1 || (n && (!a || !out || (two && !b)))) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > (size_t)G16_MAX_LAUNCH) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  g_probe_op = op; g_probe_in = in_format; g_probe_out = out_format;
  int rc = probe_ws_alloc(n, device);
  if (rc) return rc;
  rc = run_probe(probe_fmt_bytes(in_format), two ? probe_fmt_bytes(in_format) : 0, probe_fmt_bytes(out_format), (const uint8_t*)a, (const uint8_t*)b, (uint8_t*)out, n, device,
                 [](const uint8_t* x, const uint8_t* y, uint8_t* o, size_t m) { return bn254_launch_dbg_fp12_op_fmt(g_probe_op, x, y, o, m, g_probe_ws, g_probe_kinds, g_probe_in, g_probe_out, nullptr); });
  probe_ws_free();
  return rc;
}
int bn254_dbg_fp12_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int device) {
  // the entry as it always was: ops 0 .. 4 (anything else: frob1), b read for the product only
  const int o = op >= 0 && op <= 3 ? op : 4;
  return bn254_dbg_fp12_op_fmt(o, a, o == 0 ? b : nullptr, out, n, 0, 0, device);
}
// op numbers of bn254_dbg_coop12_op (include/bn254_verify.h lists them; bn254_coop12.hip::k_coop12_dbg_op takes them as they are)
enum { C12_DBG_MUL = 0, C12_DBG_MUL_CONJ_A = 2, C12_DBG_CYCLO_SQR_N = 4, C12_DBG_FROB = 5, C12_DBG_MUL_LINE_FP = 8, C12_DBG_MUL_LINE_FP2 = 10, C12_DBG_FINAL_EXP = 11, C12_DBG_EQ = 12 };
static thread_local int g_probe_arg = 0;
static thread_local DevBuf<int32_t> g_probe_target;
int bn254_dbg_coop12_op(int op, const void* a, const void* b, void* out, size_t n, int in_format, int out_format, int arg, int device) {
  const bool two = op <= C12_DBG_MUL_CONJ_A || (op >= C12_DBG_MUL_LINE_FP && op <= C12_DBG_MUL_LINE_FP2);
  if (op < 0 || op > C12_DBG_FINAL_EXP || (in_format | out_format) & ~1 || n == 0 || !a || !out || (two && !b) || (op == C12_DBG_CYCLO_SQR_N && (arg < 1 || arg > 64)) ||
      (op == C12_DBG_FROB && (arg < 1 || arg > 3)))
    return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > bn254_coop_max_proofs()) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  g_probe_op = op; g_probe_in = in_format; g_probe_out = out_format; g_probe_arg = arg;
  int rc = probe_ws_alloc(n, device);
  if (rc) return rc;
  rc = run_probe(probe_fmt_bytes(in_format), two ? probe_fmt_bytes(in_format) : 0, probe_fmt_bytes(out_format), (const uint8_t*)a, (const uint8_t*)b, (uint8_t*)out, n, device,
                 [](const uint8_t* x, const uint8_t* y, uint8_t* o, size_t m) {
                   const int kind = g_probe_in ? 3 : 0;
                   (void)hipMemsetAsync(g_probe_ws, 0, m * (size_t)G16_WS_BYTES_PER_PROOF, nullptr);    // VE_S1 of the one-operand operations: zeros, not stale words
                   hipError_t e = bn254_launch_dbg_load(g_probe_ws, m, g_probe_kinds, (int)VE_F, x, kind, nullptr);
                   if (e == hipSuccess && y) e = bn254_launch_dbg_load(g_probe_ws, m, g_probe_kinds, (int)VE_S1, y, kind, nullptr);
                   if (e == hipSuccess) e = bn254_coop12_dbg_op(g_probe_ws, g_probe_kinds, m, g_probe_op, g_probe_arg, nullptr, nullptr);
                   if (e == hipSuccess) e = bn254_launch_dbg_store(g_probe_ws, m, (int)VE_S0, o, g_probe_out, nullptr);
                   return e;
                 });
  probe_ws_free();
  return rc;
}
int bn254_dbg_verdict(int form, const void* a, const void* b, const uint8_t target[384], uint8_t* out_status, size_t n, int in_format, int device) {
  if (form < 0 || form > 2 || in_format & ~1 || n == 0 || !a || (form == 1 && !b) || !target || !out_status) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > (form == 2 ? bn254_coop_max_proofs() : (size_t)G16_MAX_LAUNCH)) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  // the target as a key holds it (bn254_host.hpp::put_fp12): reduced digits of the Montgomery form, k-order
  int32_t tgt[12 * BN_NL];
  {
    Fp12 t;
    const int korder[6] = {0, 2, 4, 1, 3, 5};
    Fp2* k[6] = {&K0(t), &K1(t), &K2(t), &K3(t), &K4(t), &K5(t)};
    for (int i = 0; i < 6; i++) {
      for (int hf = 0; hf < 2; hf++) {
        uint32_t w[8];
        words_from_be(w, target + 64 * i + 32 * hf);
        if (words_ge(w, BN_P_WORDS)) return set_err(BN254_E_BAD_ARG, "target is not canonical");
      }
      k[korder[i]]->c0 = fp_from_be(target + 64 * i); k[korder[i]]->c1 = fp_from_be(target + 64 * i + 32);
    }
    put_fp12(tgt, t);
  }
  g_probe_op = form; g_probe_in = in_format;
  int rc = probe_ws_alloc(n, device);
  if (rc) return rc;
  if ((rc = g_probe_target.ensure(12 * BN_NL))) { probe_ws_free(); return rc; }
  hipError_t ce = hipMemcpy(g_probe_target, tgt, sizeof tgt, hipMemcpyHostToDevice);
  if (ce != hipSuccess) { probe_ws_free(); g_probe_target.release(); return set_err(BN254_E_HIP, std::string("probe copy: ") + hipGetErrorString(ce)); }
  rc = run_probe(probe_fmt_bytes(in_format), form == 1 ? probe_fmt_bytes(in_format) : 0, 1, (const uint8_t*)a, (const uint8_t*)b, out_status, n, device,
                 [](const uint8_t* x, const uint8_t* y, uint8_t* o, size_t m) {
                   const int kind = g_probe_in ? 3 : 0, form = g_probe_op;
                   // where the product holds the operands: k_g16_compare reads VE_S0; k_f12_mul_verdict multiplies VE_S2 by VE_S0; the cooperative probe reads VE_F
                   hipError_t e = bn254_launch_dbg_load(g_probe_ws, m, g_probe_kinds, form == 0 ? (int)VE_S0 : form == 1 ? (int)VE_S2 : (int)VE_F, x, kind, nullptr);
                   if (e == hipSuccess && form == 1) e = bn254_launch_dbg_load(g_probe_ws, m, g_probe_kinds, (int)VE_S0, y, kind, nullptr);
                   if (e == hipSuccess) e = form == 2 ? bn254_coop12_dbg_op(g_probe_ws, g_probe_kinds, m, C12_DBG_EQ, 0, g_probe_target, nullptr)
                                                      : bn254_launch_dbg_verdict(form, g_probe_ws, m, g_probe_kinds, g_probe_target, nullptr);
                   if (e == hipSuccess) e = hipMemcpyAsync(o, g_probe_kinds, m, hipMemcpyDeviceToDevice, nullptr);
                   return e;
                 });
  probe_ws_free(); g_probe_target.release();
  return rc;
}
// the cooperative kernels in their store modes with a prepared key's line tables
static int probe_key_dev(const bn254_g16_pvk* pvk, int device, DevState** out) {
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  int rc = ensure_dev(pvk, *d, device, 1);
  if (rc) return rc;
  *out = d;
  return BN254_OK;
}
int bn254_dbg_coop12_miller_fixed(const bn254_g16_pvk* pvk, int n_pairs, const uint8_t* g1_0, const uint8_t* g1_1, const uint8_t* identity, uint8_t* out_gt, size_t n, int device) {
  if (!pvk || n_pairs < 1 || n_pairs > 2 || !g1_0 || (n_pairs == 2 && !g1_1) || !out_gt || n == 0) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > bn254_coop_max_proofs_fixed()) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  DevState* d;
  int rc = probe_key_dev(pvk, device, &d);
  if (rc) return rc;
  if ((rc = probe_ws_alloc(n, device))) return rc;
  DevBuf<uint8_t> in, out;
  std::vector<uint8_t> st(n);
  for (size_t i = 0; i < n; i++) st[i] = (uint8_t)(BN254_ST_PENDING | (identity && (identity[i] & 1) ? BN254_ST_LINF : 0) | (identity && (identity[i] & 2) ? BN254_ST_LINF2 : 0));
  auto run = [&]() -> int {
    int r;
    if ((r = in.ensure(128 * n)) || (r = out.ensure(384 * n))) return r;
    HIPCK(hipMemsetAsync(g_probe_ws, 0, n * (size_t)G16_WS_BYTES_PER_PROOF, nullptr));
    HIPCK(hipMemcpy(in, g1_0, 64 * n, hipMemcpyHostToDevice));
    if (n_pairs == 2) HIPCK(hipMemcpy(in + 64 * n, g1_1, 64 * n, hipMemcpyHostToDevice));
    hipError_t e = bn254_launch_dbg_load(g_probe_ws, n, g_probe_kinds, (int)VE_LX, in, 4, nullptr);
    if (e == hipSuccess && n_pairs == 2) e = bn254_launch_dbg_load(g_probe_ws, n, g_probe_kinds, (int)VE_CX, in + 64 * n, 4, nullptr);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("probe launch: ") + hipGetErrorString(e));
    HIPCK(hipMemcpy(g_probe_kinds, st.data(), n, hipMemcpyHostToDevice));      // after the loads (same stream): they set PENDING alone
    // the arguments of bn254_launch_pairing2_fixed's cooperative call, without the target
    e = bn254_coop12_miller_fixed(g_probe_ws, g_probe_kinds, n, n_pairs, d->gtab, d->dtab, nullptr, 0, nullptr);
    if (e == hipSuccess) e = bn254_launch_dbg_store(g_probe_ws, n, (int)VE_S0, out, 0, nullptr);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("probe launch: ") + hipGetErrorString(e));
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpy(out_gt, out, 384 * n, hipMemcpyDeviceToHost));
    return BN254_OK;
  };
  rc = run();
  probe_ws_free();
  return rc;
}
int bn254_dbg_coop12_miller_g16(const bn254_g16_pvk* pvk, const uint8_t* proofs, const uint8_t* public_inputs, size_t n_public, size_t n, uint8_t* out_gt, uint8_t* out_status,
                                int device) {
  if (!pvk || !proofs || (n_public && !public_inputs) || !out_gt || !out_status || n == 0 || n_public > (size_t)G16_WIDE_MSM_MIN_INPUTS) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > bn254_coop_max_proofs()) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  if (!pvk->host.inputs_match(n_public)) return set_err(BN254_E_BAD_ARG, "the key takes another number of public inputs");
  DevState* d;
  int rc = probe_key_dev(pvk, device, &d);
  if (rc) return rc;
  if ((rc = probe_ws_alloc(n, device))) return rc;
  DevBuf<uint8_t> in, out;
  auto run = [&]() -> int {
    int r;
    const size_t pb = 256 * n, ib = 32 * n_public * n;
    if ((r = in.ensure(pb + ib + 4)) || (r = out.ensure(384 * n))) return r;
    HIPCK(hipMemsetAsync(g_probe_ws, 0, n * (size_t)G16_WS_BYTES_PER_PROOF, nullptr));
    HIPCK(hipMemcpy(in, proofs, pb, hipMemcpyHostToDevice));
    if (ib) HIPCK(hipMemcpy(in + pb, public_inputs, ib, hipMemcpyHostToDevice));
    G16LaunchArgs a;
    a.proofs = in; a.stride = 256; a.inputs = in + pb; a.n_public = (int)n_public; a.n = n; a.ws = g_probe_ws; a.status = g_probe_kinds;
    a.msm_tab = d->msm; a.k0 = d->k0; a.gtab = d->gtab; a.dtab = d->dtab; a.target = nullptr; a.inputs_match_key = 1; a.msm_part = nullptr;
    hipError_t e = bn254_launch_dbg_coop12_g16(a, nullptr);
    if (e == hipSuccess) e = bn254_launch_dbg_store(g_probe_ws, n, (int)VE_S0, out, 0, nullptr);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("probe launch: ") + hipGetErrorString(e));
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpy(out_gt, out, 384 * n, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(out_status, g_probe_kinds, n, hipMemcpyDeviceToHost));
    // a proof the loader passed keeps PENDING (with a deferred error of C in the low bits, which the pairing does not look at): it reached the pairing
    for (size_t i = 0; i < n; i++) if (out_status[i] & BN254_ST_PENDING) out_status[i] = (out_status[i] & 0x3f) ? (uint8_t)(out_status[i] & 0x3f) : (uint8_t)BN254_ACCEPT;
    return BN254_OK;
  };
  rc = run();
  probe_ws_free();
  return rc;
}
// ---- the Groth16 loader stage by value (include/bn254_verify.h: bn254_dbg_g16_loader, bn254_dbg_g16_loader_keys) ----------------------------------------------------
// What the stage left in the workspace, read through k_dbg_store from VE_AX on: twelve elements in the store's order -- (AX, AY), B.y, (LX, LY), B.x, (CX, CY), two
// more -- turned into the 320 bytes A | B (x.c1 x.c0 y.c1 y.c0, as a record holds it) | C | L of every item
#define G16_LOADER_PROBE_MAX 32768
static void g16_loader_points(const uint8_t* stored, size_t m, uint8_t* out) {
  for (size_t i = 0; i < m; i++) {
    const uint8_t* p = stored + 384 * i;
    uint8_t* o = out + 320 * i;
    memcpy(o, p, 64);                                                   // A
    memcpy(o + 64, p + 192 + 32, 32); memcpy(o + 96, p + 192, 32);      // B.x: c1, c0
    memcpy(o + 128, p + 64 + 32, 32); memcpy(o + 160, p + 64, 32);      // B.y: c1, c0
    memcpy(o + 192, p + 256, 64);                                       // C
    memcpy(o + 256, p + 128, 64);                                       // L
  }
}
int bn254_dbg_g16_loader(const bn254_g16_pvk* pvk, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs, size_t n_public, size_t n, unsigned flags, int form,
                         int misalign, uint8_t* out_status, uint8_t* out_slot_status, unsigned* out_slot_proof, uint8_t* out_points, int info[6], int device) {
  if (!pvk || !proofs || (n_public && !public_inputs) || !out_status || !out_points || !info || n == 0 || proof_stride < 256 || proof_stride > 4096 || n_public > 4096 ||
      form < 0 || form > 3 || misalign < 0 || misalign > 3 || (flags & ~(unsigned)BN254_FLAG_STRICT_SCALARS) || (form == 1 && (!out_slot_status || !out_slot_proof)))
    return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > (size_t)G16_LOADER_PROBE_MAX) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  // a combination bn254_launch_g16 could never reach is refused: the plan's own predicates, with the form in the place of the sizes and the knobs
  const size_t key_inputs = pvk->host.key_inputs();
  const bool match = pvk->host.inputs_match(n_public), strict = (flags & BN254_FLAG_STRICT_SCALARS) != 0;
  const bool wide = form >= 2;
  const int per = g16_wide_per(knob_wide_per()), chunks = wide ? g16_wide_chunks(n_public, per) : 0;
  if (wide ? !(match && n_public > (size_t)G16_WIDE_MSM_MIN_INPUTS) : (match && n_public > (size_t)G16_WIDE_MSM_MIN_INPUTS))
    return set_err(BN254_E_BAD_ARG, wide ? "the wide forms take a key with more than 16 inputs and its own input count" : "a key with more than 16 inputs sums them in the wide forms");
  if (form == 1 && !(g16_key_may_compact(key_inputs) && !strict)) return set_err(BN254_E_BAD_ARG, "no launch compacts for this key and these flags");
  if (form == 3 && !g16_wide_reduce8((size_t)chunks, n)) return set_err(BN254_E_BAD_ARG, "k_g16_msm_reduce8 is launched from 16 chunk sums per proof on");
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  int rc = ensure_dev(pvk, *d, device, n);
  if (rc) return rc;
  if ((rc = probe_ws_alloc(n, device))) return rc;
  DevBuf<uint8_t> in, out;
  auto run = [&]() -> int {
    int r;
    const size_t pb = (n - 1) * proof_stride + 256, pb4 = (pb + 3) & ~(size_t)3, ib = 32 * n_public * n;
    if ((r = in.ensure(pb4 + ib + 8)) || (r = out.ensure(384 * n))) return r;
    HIPCK(hipDeviceSynchronize());                                     // the key's buffers may still serve an earlier batch on another stream
    HIPCK(hipMemsetAsync(g_probe_ws, 0, n * (size_t)G16_WS_BYTES_PER_PROOF, nullptr));
    HIPCK(hipMemsetAsync(g_probe_kinds, 0xEE, n, nullptr));            // the caller's status buffer holds whatever it held: the stage writes every byte
    HIPCK(hipMemcpy(in, proofs, pb, hipMemcpyHostToDevice));
    if (ib) HIPCK(hipMemcpy(in + pb4 + misalign, public_inputs, ib, hipMemcpyHostToDevice));
    G16LaunchArgs a;
    a.proofs = in; a.stride = proof_stride; a.inputs = in + pb4 + misalign; a.n_public = (int)n_public; a.n = n; a.ws = g_probe_ws; a.status = g_probe_kinds;
    a.msm_tab = d->msm; a.k0 = d->k0; a.gtab = d->gtab; a.dtab = d->dtab; a.target = d->target; a.inputs_match_key = match ? 1 : 0; a.strict_scalars = strict ? 1 : 0;
    a.msm_comb = pvk->host.msm_comb ? 1 : 0; a.msm_part = nullptr; a.key_inputs = key_inputs;
    if (wide) {
      if (n > d->msm_part_cap || (size_t)chunks > d->msm_chunks) return set_err(BN254_E_BAD_ARG, "partial-sum buffer smaller than the batch (internal sizing error)");
      a.msm_part = (int32_t*)d->msm_part;
      if (pvk->host.msm_comb) a.msm_digits = (uint16_t*)(d->msm_part + d->msm_chunks * 27 * d->msm_part_cap);
    }
    if (form == 1) {
      if (n > d->compact_cap) return set_err(BN254_E_BAD_ARG, "slot arrays smaller than the batch (internal sizing error)");
      const G16CompactAlloc ca = g16_compact_alloc(d->compact_cap, key_inputs);
      a.slot_proof = (uint32_t*)d->compact;
      a.block_count = (uint32_t*)d->compact + ca.slot_proof_bytes / 4;
      a.slot_status = (uint8_t*)((uint32_t*)d->compact + (ca.slot_proof_bytes + ca.count_bytes) / 4);
    }
    G16LoaderForm f;
    f.wide = wide; f.coop = false; f.compact = form == 1; f.reduce = form == 3 ? G16_REDUCE_EIGHT : G16_REDUCE_PLAIN;
    G16LoaderRan ran;
    bn254_launch_g16_loader(a, f, nullptr, nullptr, &ran);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = bn254_launch_dbg_store(g_probe_ws, n, (int)VE_AX, out, 0, nullptr);
    if (e != hipSuccess) return set_err(BN254_E_HIP, std::string("probe launch: ") + hipGetErrorString(e));
    HIPCK(hipDeviceSynchronize());
    std::vector<uint8_t> stored(384 * n);
    HIPCK(hipMemcpy(stored.data(), out, 384 * n, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(out_status, g_probe_kinds, n, hipMemcpyDeviceToHost));
    if (form == 1) {
      HIPCK(hipMemcpy(out_slot_status, a.slot_status, n, hipMemcpyDeviceToHost));
      HIPCK(hipMemcpy(out_slot_proof, a.slot_proof, n * 4, hipMemcpyDeviceToHost));
    }
    g16_loader_points(stored.data(), n, out_points);
    // what the launcher says it enqueued, not what was asked for
    info[0] = ran.compaction ? 1 : ran.prepare_full ? 0 : ran.reduce == 2 ? 3 : ran.reduce == 1 ? 2 : -1; info[1] = ran.chunks; info[2] = ran.reduce; info[3] = ran.partial;
    info[4] = ran.check_scalars; info[5] = ran.comb_digits;
    return BN254_OK;
  };
  rc = run();
  probe_ws_free();
  return rc;
}
int bn254_dbg_g16_loader_keys(const bn254_g16_pvk* const* pvks, size_t n_keys, const unsigned* key_index, const uint8_t* proofs, size_t proof_stride, const uint8_t* public_inputs,
                              size_t input_stride, size_t n, unsigned flags, int misalign, size_t max_slots, unsigned* out_slot_proof, uint8_t* out_slot_status, uint8_t* out_points,
                              size_t* out_n_slots, int device) {
  size_t max_public = 0;
  if (!out_slot_proof || !out_slot_status || !out_points || !out_n_slots || n == 0 || misalign < 0 || misalign > 3 || (flags & ~(unsigned)BN254_FLAG_STRICT_SCALARS) ||
      proof_stride > 4096 || input_stride > 65536)
    return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n > (size_t)G16_LOADER_PROBE_MAX) return set_err(BN254_E_BAD_ARG, "probe batch too large");
  int rc = check_keys_args(pvks, n_keys, key_index, proofs, proof_stride, public_inputs, input_stride, n, out_slot_status, flags, &max_public);
  if (rc) return rc;
  size_t slots = 0;
  {
    std::vector<uint32_t> count(n_keys, 0);
    for (size_t i = 0; i < n; i++) {
      if (key_index[i] >= n_keys) return set_err(BN254_E_BAD_ARG, "key_index[" + std::to_string(i) + "] is outside the list");
      count[key_index[i]]++;
    }
    for (size_t k = 0; k < n_keys; k++) slots += bn254::keys_round_up(count[k]);
  }
  if (slots > max_slots) return set_err(BN254_E_BAD_ARG, "the batch fills more slots than the output arrays hold");
  return g16_keys_probe_loader(pvks, n_keys, key_index, proofs, proof_stride, public_inputs, input_stride, n, flags, misalign, slots, out_slot_proof, out_slot_status, out_points,
                               out_n_slots, device, g16_loader_points);
}
int bn254_dbg_pairing(const uint8_t* g1, const uint8_t* g2, uint8_t* out_gt, size_t n, int device) {
  int rc = probe_ws_alloc(n, device);
  if (rc) return rc;
  rc = run_probe(64, 128, 384, g1, g2, out_gt, n, device, [](const uint8_t* x, const uint8_t* y, uint8_t* o, size_t m) { return bn254_launch_dbg_pairing(x, y, o, m, g_probe_ws, g_probe_kinds, nullptr); });
  probe_ws_free();
  return rc;
}
int bn254_dbg_g2_subgroup_ate(const uint8_t* g1, const uint8_t* g2, uint8_t* out_flags, size_t n, int device) {
  int rc = probe_ws_alloc(n, device);
  if (rc) return rc;
  rc = run_probe(64, 128, 1, g1, g2, out_flags, n, device, [](const uint8_t* x, const uint8_t* y, uint8_t* o, size_t m) { return bn254_launch_dbg_g2_ate(x, y, o, m, g_probe_ws, g_probe_kinds, nullptr); });
  probe_ws_free();
  return rc;
}
int bn254_dbg_g2_subgroup(const uint8_t* g2, uint8_t* out_flags, size_t n, int device) {
  return run_probe(128, 0, 1, g2, nullptr, out_flags, n, device, [](const uint8_t* x, const uint8_t*, uint8_t* o, size_t m) { return bn254_launch_dbg_g2_subgroup(x, o, m, nullptr); });
}

#if defined(BN254_PLONK_MARKS)
// diagnostics build: stage 1 of ONE proof on the host, and the intermediate values it dumped (bn254_plonk.hpp::PL_DUMP): the reference the device's dump is held to
int bn254_dbg_plonk_dump_host(const bn254_plonk_pvk* pvk, const uint8_t* proof, size_t proof_len, const uint8_t* inputs, size_t n_public, uint8_t out[64 * 32], int* status) {
  if (!pvk || !proof || !out || !status) return set_err(BN254_E_BAD_ARG, "bad argument");
  PlonkWork wk; std::vector<MsmTerm> terms(plonk_stage1_terms(pvk->key)); std::vector<uint8_t> fl(terms.size());
  memset(g_plonk_dump_host, 0, sizeof g_plonk_dump_host);
  g_plonk_sha_n_host = 0;
  wk.lambda = fr_ctx().one;
  *status = plonk_stage1(pvk->key, proof, proof_len, inputs, n_public, wk, terms.data(), fl.data());
  memcpy(out, g_plonk_dump_host, 64 * 32);
  return BN254_OK;
}
int bn254_dbg_plonk_sha_dump_host(uint32_t out[32 * 24], uint32_t* n) { memcpy(out, g_plonk_sha_dump_host, sizeof g_plonk_sha_dump_host); *n = g_plonk_sha_n_host; return BN254_OK; }
#endif
// GLV decomposition probe (host only): k (32 bytes big-endian, any value: reduced mod r) -> |k1|, |k2| (16 bytes big-endian each) and signs
int bn254_dbg_glv_decompose(const uint8_t k32[32], uint8_t k1_16[16], uint8_t k2_16[16], int* neg1, int* neg2) {
  if (!k32 || !k1_16 || !k2_16 || !neg1 || !neg2) return set_err(BN254_E_BAD_ARG, "bad argument");
  const FrCtx& F = fr_ctx();
  Glv g = glv_decompose(F.to_canon(F.from_be32(k32)));
  for (int i = 0; i < 8; i++) { k1_16[i] = (uint8_t)(g.k1[1] >> (56 - 8 * i)); k1_16[8 + i] = (uint8_t)(g.k1[0] >> (56 - 8 * i)); k2_16[i] = (uint8_t)(g.k2[1] >> (56 - 8 * i)); k2_16[8 + i] = (uint8_t)(g.k2[0] >> (56 - 8 * i)); }
  *neg1 = g.neg1 ? 1 : 0; *neg2 = g.neg2 ? 1 : 0;
  return BN254_OK;
}

// host-only probe of the Fr inversion the PlonK stages use (bn254_plonk.hpp::FrCtx::inverse, binary extended GCD; which = 1: the Fermat form it replaced;
// field = 1: the same code instantiated for Fp, as the curve checks of the proof points use it).  in / out: 32-byte big-endian canonical values.
// host-only probes of the PlonK batch plan and of the scratch sizing (tests: every pass of every plan must fit the scratch of a context of its capacity)
int bn254_dbg_plonk_plan(size_t n, size_t piece, int max_workers, int* workers, size_t* per_worker, size_t* per_pass) {
  if (!workers || !per_worker || !per_pass || n == 0 || piece == 0 || max_workers < 1) return set_err(BN254_E_BAD_ARG, "bad argument");
  plonk_plan(n, piece, max_workers, workers, per_worker, per_pass);
  return BN254_OK;
}
size_t bn254_dbg_plonk_scratch_lanes(size_t capacity, int n_var) { return plonk_scratch_lanes(capacity, n_var); }
size_t bn254_dbg_plonk_part_points(size_t capacity, int n_qcp, int stage) {
  if (n_qcp < 0 || n_qcp > PLONK_MAX_QCP || stage < 1 || stage > 3) return 0;
  PlonkKey key; key.n_qcp = (uint32_t)n_qcp;
  MsmShape sh;
  if (stage == 1) plonk_msm1_shape(key, sh); else plonk_msm2_shape(key, sh, stage == 3);
  return plonk_part_points(capacity, sh);
}
// the row plan of one MSM launch of the PlonK path (stage 1: the digest; 2: the KZG check) for a key with n_qcp commitments and a batch of n proofs:
// rows, rows with a window table, scratch lanes the launch needs, the longest row in the planner's cost units, rows per sum; rows_out (optional):
// MSM_MAX_ROWS x 9 ints {variable term, pos_lo, pos_hi, unit term, sum, scratch slot, first fixed window, one past the last, joint-row term mask}
int bn254_dbg_plonk_msm_plan(int n_qcp, int stage, size_t n, size_t lane_budget, int* n_rows, int* n_var_rows, size_t* scratch_lanes, int* chain, int sum_rows[2],
                             int fixed_terms[2], int* rows_out) {
  if (n_qcp < 0 || n_qcp > PLONK_MAX_QCP || (stage != 1 && stage != 2) || n == 0 || !n_rows || !n_var_rows || !scratch_lanes || !chain || !sum_rows || !fixed_terms)
    return set_err(BN254_E_BAD_ARG, "bad argument");
  PlonkKey key; key.n_qcp = (uint32_t)n_qcp;
  MsmShape sh;
  if (stage == 1) plonk_msm1_shape(key, sh); else plonk_msm2_shape(key, sh);
  MsmPlan plan;
  if (!msm_plan_build(plan, sh, (n + 63) & ~(size_t)63, lane_budget ? lane_budget : msm_lane_budget(), 0, plonk_joint_g((n + 63) & ~(size_t)63))) return set_err(BN254_E_BAD_ARG, "shape cannot be planned");
  *n_rows = plan.n_rows; *n_var_rows = plan.n_var_rows; *scratch_lanes = bn254_g1_msm_scratch_lanes(plan, n); *chain = msm_plan_chain(plan);
  for (int k = 0; k < 2; k++) { sum_rows[k] = plan.count[k]; fixed_terms[k] = plan.n_fixed[k]; }
  if (rows_out)
    for (int r = 0; r < plan.n_rows; r++) {
      const MsmRow& w = plan.row[r];
      int* o = rows_out + 9 * r;
      o[0] = w.n_joint ? -1 : w.var_term; o[1] = w.pos_lo; o[2] = w.pos_hi; o[3] = w.unit_term; o[4] = w.sum; o[5] = w.glv_slot; o[6] = w.fw_lo; o[7] = w.fw_hi;
      o[8] = 0;                                     // a joint row: the bit mask of the terms it walks together
      for (int j = 0; j < w.n_joint; j++) o[8] |= 1 << plan.var_list[w.sum][w.var_term + j];
    }
  return BN254_OK;
}
int bn254_dbg_fr_inverse(const uint8_t in32[32], uint8_t out32[32], int which, int field) {
  if (!in32 || !out32) return set_err(BN254_E_BAD_ARG, "bad argument");
  const FrCtx& F = field ? fp64_ctx().F : fr_ctx();
  const FrM a = F.from_be_reduce(in32, 32);
  F.to_be(out32, which == 1 ? F.inverse_fermat(a) : which == 2 ? F.inverse_bgcd(a) : F.inverse(a));
  return BN254_OK;
}
// n products a_i * b_i in the field (operands: any 256-bit values, reduced and converted to Montgomery form first), through the
// product form the DEVICE stages use (form 32: eight 32-bit words) or the host's (form 64: four 64-bit limbs on __int128); out = canonical big-endian
int bn254_dbg_fr_mul(const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int form, int field) {
  if ((!a || !b || !out) && n) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (form != 32 && form != 64) return set_err(BN254_E_BAD_ARG, "form is 32 or 64");
  const FrCtx& F = field ? fp64_ctx().F : fr_ctx();
  for (size_t i = 0; i < n; i++) {
    const FrM x = F.from_be_reduce(a + 32 * i, 32), y = F.from_be_reduce(b + 32 * i, 32);
    F.to_be(out + 32 * i, form == 32 ? F.mul_w32(x, y) : F.mul_w64(x, y));
  }
  return BN254_OK;
}

// The fixed-base tables a device built for a key (bn254_k_comb.hip) against the host constructions (build_comb_table / build_window_table): the tables of the first `inputs`
// points are read back and compared entry by entry as field values.  *mismatches = entries that differ (0: identical); needs a device.
static int compare_tables(int form, const std::vector<int32_t>& pts, const int32_t* d_tab, int inputs, size_t* mismatches) {
  const size_t np = pts.size() / (2 * BN_NL), n_entries = form == 0 ? ((size_t)1 << G16_COMB_TEETH) : (size_t)32 * 255, per = n_entries * MSM_ENTRY_DWORDS;
  if ((size_t)inputs > np) inputs = (int)np;
  std::vector<int32_t> dev_tab((size_t)inputs * per), host_tab(per);
  HIPCK(hipMemcpy(dev_tab.data(), d_tab, dev_tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  size_t bad = 0;
  for (int i = 0; i < inputs; i++) {
    G1Aff K; K.x = fp_from_limbs(pts.data() + (size_t)i * 2 * BN_NL); K.y = fp_from_limbs(pts.data() + (size_t)i * 2 * BN_NL + BN_NL);
    if (form == 0) build_comb_table(host_tab.data(), K); else build_window_table(host_tab.data(), K);
    for (size_t e = form == 0 ? 1 : 0; e < n_entries; e++) {
      const int32_t* a = dev_tab.data() + (size_t)i * per + e * MSM_ENTRY_DWORDS; const int32_t* b = host_tab.data() + e * MSM_ENTRY_DWORDS;
      if (!fp_eq(fp_from_limbs(a), fp_from_limbs(b)) || !fp_eq(fp_from_limbs(a + BN_NL), fp_from_limbs(b + BN_NL)) || a[18] != 0 || a[19] != 0) bad++;
    }
  }
  *mismatches = bad;
  return BN254_OK;
}
// window tables of MSM_FW_BITS bits (form 2): MSM_FW_WINDOWS x (2^MSM_FW_BITS - 1) entries per point: every window's first, middle and last entries and a pseudo-random
// sample, each against d 2^(bits w) P by double-and-add
static int compare_window_tables(const std::vector<int32_t>& pts, const int32_t* d_tab, size_t* mismatches) {
  const size_t np = pts.size() / (2 * BN_NL), per = (size_t)MSM_FW_WINDOWS * MSM_FW_ENTRIES;
  size_t bad = 0;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  std::vector<int32_t> e(MSM_ENTRY_DWORDS);
  for (size_t i = 0; i < np; i++) {
    G1Aff P; P.x = fp_from_limbs(pts.data() + i * 2 * BN_NL); P.y = fp_from_limbs(pts.data() + i * 2 * BN_NL + BN_NL);
    G1Proj bw = g1_from_affine(P);
    for (int w = 0; w < MSM_FW_WINDOWS; w++) {
      std::vector<uint32_t> ds = {1, 2, 3, 255 % MSM_FW_ENTRIES + 1, 256 % MSM_FW_ENTRIES + 1, (MSM_FW_ENTRIES >> 1), (MSM_FW_ENTRIES >> 1) + 1, MSM_FW_ENTRIES - 1, MSM_FW_ENTRIES};
      for (int k = 0; k < 14; k++) { x ^= x >> 12; x ^= x << 25; x ^= x >> 27; ds.push_back(1 + (uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 40) % MSM_FW_ENTRIES); }
      for (uint32_t dd : ds) {
        HIPCK(hipMemcpy(e.data(), d_tab + (i * per + (size_t)w * MSM_FW_ENTRIES + dd - 1) * MSM_ENTRY_DWORDS, MSM_ENTRY_DWORDS * sizeof(int32_t), hipMemcpyDeviceToHost));
        G1Proj acc = g1_identity();
        for (int bit = MSM_FW_BITS - 1; bit >= 0; bit--) { acc = g1_dbl(acc); if ((dd >> bit) & 1) acc = g1_add(acc, bw); }
        const G1Aff want = g1_to_affine(acc);
        if (!fp_eq(fp_from_limbs(e.data()), want.x) || !fp_eq(fp_from_limbs(e.data() + BN_NL), want.y) || e[18] != 0 || e[19] != 0) bad++;
      }
      for (int b = 0; b < MSM_FW_BITS; b++) bw = g1_dbl(bw);
    }
  }
  *mismatches = bad;
  return BN254_OK;
}
int bn254_dbg_comb_table_compare(const bn254_g16_pvk* pvk, int device, int inputs, size_t* mismatches) {
  if (!pvk || !mismatches || inputs < 1) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (pvk->host.kpts.empty()) return set_err(BN254_E_BAD_ARG, "the key's tables were not built on the device");
  DevState* d = dev_state(pvk, device);
  std::lock_guard<std::mutex> lk(d->mu);
  int rc = ensure_dev(pvk, *d, device, 1);
  if (rc) return rc;
  const int form = g16_table_form(pvk->host);
  if (form == 2) return compare_window_tables(pvk->host.kpts, d->msm, mismatches);
  return compare_tables(form, pvk->host.kpts, d->msm, inputs, mismatches);
}
int bn254_dbg_plonk_table_compare(const bn254_plonk_pvk* pvk, int device, size_t* mismatches) {
  if (!pvk || !mismatches) return set_err(BN254_E_BAD_ARG, "bad argument");
  PlonkDev* d;
  std::lock_guard<std::mutex> lk(pvk->mu);
  int rc = plonk_ensure_dev(pvk, device, &d);
  if (rc) return rc;
  return compare_window_tables(pvk->fixed_pts, d->fixed_tabs, mismatches);
}
// host-only probe of the comb tables of keys with many public inputs: x * P from build_comb_table(P) and the column digits the kernels use
int bn254_dbg_comb_mul(const uint8_t p64[64], const uint8_t x32[32], uint8_t out64[64]) {
  if (!p64 || !x32 || !out64) return set_err(BN254_E_BAD_ARG, "bad argument");
  G1Aff P; P.x = fp_from_be(p64); P.y = fp_from_be(p64 + 32);
  if (!g1_on_curve(P)) return set_err(BN254_E_BAD_ARG, "not a curve point");
  std::vector<int32_t> tab(((size_t)1 << G16_COMB_TEETH) * MSM_ENTRY_DWORDS);
  build_comb_table(tab.data(), P);
  uint32_t w[8];
  for (int k = 0; k < 8; k++) { const uint8_t* q = x32 + 28 - 4 * k; w[k] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3]; }
  G1Proj acc = g1_identity();
  for (int col = G16_COMB_COLS - 1; col >= 0; col--) {
    acc = g1_dbl(acc);
    const uint32_t idx = g16_comb_digit(w, col);
    if (idx) {
      G1Aff e; e.x = fp_from_limbs(tab.data() + (size_t)idx * MSM_ENTRY_DWORDS); e.y = fp_from_limbs(tab.data() + (size_t)idx * MSM_ENTRY_DWORDS + BN_NL);
      acc = g1_add_mixed(acc, e);
    }
  }
  if (g1_is_identity(acc)) { memset(out64, 0, 64); return BN254_OK; }
  enc_g1_uncompressed(out64, g1_to_affine(acc));
  return BN254_OK;
}

// ---------------------------------------------------------------- value-level probes of the G1 layer of the PlonK path (tests/test_gpu_g1_msm_values.py)
// k_g1_msm_rows[_keys], k_g1_sum_affine, k_plonk_group_sums / _scatter through the launchers the product calls, on data the caller places.  Every argument is
// checked here, on the host, before the device is looked at: nothing a kernel reads -- an index, a count, a digit -- is taken on trust.
namespace {
enum { G1P_MAX_MSM_ITEMS = 32768, G1P_MAX_ITEMS = 65536, G1P_MAX_TERMS = 64, G1P_MAX_BASES = 32, G1P_MAX_KEYS = 8 };
inline uint32_t g1p_be_word(const uint8_t* q) { return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3]; }
inline uint32_t g1p_le_word(const uint8_t* q) { return (uint32_t)q[3] << 24 | (uint32_t)q[2] << 16 | (uint32_t)q[1] << 8 | (uint32_t)q[0]; }
// what k_g1_sum_affine declares for a row it loads (BN_SETB(t, 3.0, 0.5)), exactly: the eight low digits in [-2^28, 2^28] and |value| <= 3 p.  3 p -+ v is carried
// with floor shifts, so the sign of the number is the sign of what arrives at the top digit.
bool g1p_row_digits_ok(const int32_t* d) {
  for (int i = 0; i < BN_NL - 1; i++) if (d[i] < -BN_HALF || d[i] > BN_HALF) return false;
  for (int sign = -1; sign <= 1; sign += 2) {
    int64_t c = 0;
    for (int i = 0; i < BN_NL - 1; i++) c = (c + 3 * (int64_t)bn_p_limb(i) + sign * (int64_t)d[i]) >> BN_LB;
    if (c + 3 * (int64_t)bn_p_limb(BN_NL - 1) + sign * (int64_t)d[BN_NL - 1] < 0) return false;
  }
  return true;
}
// the int encoding of tests/hostsim's hs_msm_rows_joint, every index against its list; kind[t]: bit 0 variable, 1 unit, 2 fixed
bool g1p_parse_shape(const int* q, size_t len, size_t n_terms, size_t n_bases, MsmShape& sh, uint8_t* kind) {
  memset(&sh, 0, sizeof sh);
  memset(kind, 0, n_terms);
  if (len < 1 || q[0] < 1 || q[0] > 2 || len < 1 + 3 * (size_t)q[0]) return false;
  sh.n_sums = q[0];
  size_t need = 1 + 3 * (size_t)sh.n_sums;
  for (int s = 0; s < sh.n_sums; s++) {
    const int v = q[1 + 3 * s], u = q[2 + 3 * s], f = q[3 + 3 * s];
    if (v < 0 || v > MSM_MAX_FIXED || u < 0 || u > 4 || f < 0 || f > MSM_MAX_FIXED) return false;
    sh.n_var[s] = v; sh.n_unit[s] = u; sh.n_fixed[s] = f;
    need += (size_t)v + (size_t)u + 2 * (size_t)f;
  }
  if (len != need) return false;
  const int* p = q + 1 + 3 * sh.n_sums;
  auto term = [&](int t, uint8_t bit) { if (t < 0 || (size_t)t >= n_terms) return false; kind[t] |= bit; return true; };
  for (int s = 0; s < sh.n_sums; s++) {
    for (int i = 0; i < sh.n_var[s]; i++, p++) { if (!term(*p, 1)) return false; sh.var_term[s][i] = (int8_t)*p; }
    for (int i = 0; i < sh.n_unit[s]; i++, p++) { if (!term(*p, 2)) return false; sh.unit_term[s][i] = (int8_t)*p; }
    for (int i = 0; i < sh.n_fixed[s]; i++, p++) { if (!term(*p, 4)) return false; sh.fixed_term[s][i] = (int8_t)*p; }
    for (int i = 0; i < sh.n_fixed[s]; i++, p++) { if (*p < 0 || (size_t)*p >= n_bases) return false; sh.fixed_tab[s][i] = (int8_t)*p; }
  }
  for (size_t t = 0; t < n_terms; t++) if ((kind[t] & 4) && (kind[t] & 3)) return false;      // a record's scalar words are its GLV halves OR its fixed scalar
  return true;
}
int g1p_plan_form(const MsmPlan& p) {
  bool split = false;
  for (int r = 0; r < p.n_rows; r++) {
    if (p.row[r].n_joint) return 2;
    if (p.row[r].var_term >= 0 && (p.row[r].pos_lo != 0 || p.row[r].pos_hi != 128)) split = true;
  }
  return split ? 0 : 1;
}
// n affine points of 64 bytes: every coordinate below p
bool g1p_points_canonical(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < 2 * n; i++) if (!be_lt_p(p + 32 * i)) return false;
  return true;
}
inline void g1p_words_point(uint8_t* out64, const uint32_t* w16, bool inf) {
  if (inf) { memset(out64, 0, 64); return; }
  words_to_be(out64, w16); words_to_be(out64 + 32, w16 + 8);
}
// k_g1_sum_affine over `part` (the plan's rows x 27 x n dwords on the device) in one of the two output modes of the probes
int g1p_sum_and_fetch(const MsmPlan& plan, const int32_t* part, size_t n, int out_mode, uint8_t* out_points, uint8_t* out_inf, uint8_t* status) {
  int rc;
  const int n_sums = plan.count[1] > 0 ? 2 : 1;
  if (out_mode == 0) {
    DevBuf<uint32_t> words; DevBuf<uint8_t> inf;
    if ((rc = words.ensure(16 * n)) || (rc = inf.ensure(n))) return rc;
    std::vector<uint32_t> hw(16 * n); std::vector<uint8_t> hi(n);
    for (int s = 0; s < n_sums; s++) {
      MsmPlan one = plan;                                   // the words form of the kernel holds one sum per item: sum s alone
      one.first[0] = plan.first[s]; one.count[0] = plan.count[s]; one.first[1] = 0; one.count[1] = 0;
      hipError_t e = bn254_launch_g1_sum_rows(one, part, n, words, inf, nullptr, nullptr, 0, 0, 0, 0, nullptr);
      if (e != hipSuccess) return launch_err(e, "probe");
      HIPCK(hipDeviceSynchronize());
      HIPCK(hipMemcpy(hw.data(), words, hw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      HIPCK(hipMemcpy(hi.data(), inf, n, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; i++) {
        out_inf[i * n_sums + s] = hi[i];
        g1p_words_point(out_points + 64 * (i * n_sums + s), hw.data() + 16 * i, hi[i] != 0);
      }
    }
    return BN254_OK;
  }
  DevBuf<int32_t> ws; DevBuf<uint8_t> st, out;
  const size_t st_bytes = (n + 3) & ~(size_t)3;             // the identity flags are OR-ed into whole status words
  if ((rc = ws.ensure(n * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = st.ensure(st_bytes)) || (rc = out.ensure(384 * n))) return rc;
  HIPCK(hipMemset(ws, 0, n * (size_t)G16_WS_BYTES_PER_PROOF));
  HIPCK(hipMemset(st, 0, st_bytes));
  HIPCK(hipMemcpy(st, status, n, hipMemcpyHostToDevice));
  hipError_t e = bn254_launch_g1_sum_rows(plan, part, n, nullptr, nullptr, ws, st, VE_LX_ELEM, BN254_ST_LINF, VE_CX_ELEM, BN254_ST_LINF2, nullptr);   // plonk_msm's call
  // elements 6 .. 17 as one Fp12 in the store's byte order: (VE_CX, VE_CY) first, (VE_LX, VE_LY) fourth
  if (e == hipSuccess) e = bn254_launch_dbg_store(ws, n, (int)VE_CX_ELEM, out, 0, nullptr);
  if (e != hipSuccess) return launch_err(e, "probe");
  HIPCK(hipDeviceSynchronize());
  std::vector<uint8_t> ho(384 * n);
  HIPCK(hipMemcpy(ho.data(), out, ho.size(), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(status, st, n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) { memcpy(out_points + 128 * i, ho.data() + 384 * i + 192, 64); memcpy(out_points + 128 * i + 64, ho.data() + 384 * i, 64); }
  return BN254_OK;
}
}  // namespace
static_assert(VE_LX_ELEM == VE_CX_ELEM + 2, "the workspace store of the G1 probes reads both points as one Fp12 at VE_CX");

int bn254_dbg_g1_msm(const int* shape, size_t shape_ints, const uint8_t* terms, size_t n_terms, const uint8_t* bases, size_t n_bases, size_t n_keys, const unsigned* granule_key,
                     size_t n, size_t lane_budget, int joint_g, int out_mode, uint8_t* out_points, uint8_t* out_inf, uint8_t* status, int info[6], int device) {
  if (!shape || !terms || !bases || !out_points || !info || (out_mode == 0 && !out_inf) || (out_mode == 1 && !status) || (out_mode & ~1)) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n == 0 || n > (size_t)G1P_MAX_MSM_ITEMS) return set_err(BN254_E_BAD_ARG, "bad argument: n is 1 .. 32768");
  if (n_terms == 0 || n_terms > (size_t)G1P_MAX_TERMS || n_bases == 0 || n_bases > (size_t)G1P_MAX_BASES || n_keys == 0 || n_keys > (size_t)G1P_MAX_KEYS)
    return set_err(BN254_E_BAD_ARG, "bad argument: up to 64 terms, 32 bases, 8 keys");
  if ((lane_budget && lane_budget < 64) || joint_g < 0 || joint_g > MSM_MAX_JOINT) return set_err(BN254_E_BAD_ARG, "bad argument: lane_budget is 0 or at least 64, joint_g 0 .. 8");
  const size_t n_pad = (n + 63) & ~(size_t)63, granules = n_pad / 64;
  if (n_keys > 1) {
    if (!granule_key) return set_err(BN254_E_BAD_ARG, "bad argument: a key list needs the granules' key indices");
    for (size_t g = 0; g < granules; g++) if (granule_key[g] >= n_keys) return set_err(BN254_E_BAD_ARG, "bad argument: key index outside the list");
  }
  MsmShape sh;
  uint8_t kind[G1P_MAX_TERMS];
  if (!g1p_parse_shape(shape, shape_ints, n_terms, n_bases, sh, kind)) return set_err(BN254_E_BAD_ARG, "bad argument: shape (a count, a term index or a table index outside its list)");
  MsmPlan plan;
  if (!msm_plan_build(plan, sh, n_pad, lane_budget ? lane_budget : msm_lane_budget(), 0, joint_g) || plan.n_rows > MSM_MAX_ROWS)
    return set_err(BN254_E_BAD_ARG, "bad argument: the shape needs more MSM rows than a launch has");
  for (size_t k = 0; k < n_keys * n_bases; k++) {
    G1Aff K; K.x = fp_from_be(bases + 64 * k); K.y = fp_from_be(bases + 64 * k + 32);
    if (!g1p_points_canonical(bases + 64 * k, 1) || !g1_on_curve(K)) return set_err(BN254_E_BAD_ARG, "bad argument: a base is not a curve point");
  }
  // the records as the stage kernels leave them: MsmTerm digits and scalar words, flag bytes
  std::vector<int32_t> ht(n * n_terms * (size_t)MSM_TERM_DWORDS, 0);
  std::vector<uint8_t> hf(n * n_terms);
  for (size_t k = 0; k < n * n_terms; k++) {
    const uint8_t* e = terms + 129 * k;
    int32_t* o = ht.data() + k * (size_t)MSM_TERM_DWORDS;
    hf[k] = e[128];
    if (kind[k % n_terms] & 4) { for (int w = 0; w < 8; w++) o[18 + w] = (int32_t)g1p_le_word(e + 96 + 4 * w); continue; }
    if (!g1p_points_canonical(e, 1)) return set_err(BN254_E_BAD_ARG, "bad argument: a coordinate of a term's point is not below p");
    fp_to_limbs(o, fp_from_be(e)); fp_to_limbs(o + BN_NL, fp_from_be(e + 32));
    for (int w = 0; w < 4; w++) { o[18 + w] = (int32_t)g1p_be_word(e + 64 + 4 * (3 - w)); o[22 + w] = (int32_t)g1p_be_word(e + 80 + 4 * (3 - w)); }
  }
  info[0] = plan.n_rows; info[1] = plan.n_var_rows; info[2] = plan.count[0]; info[3] = plan.count[1]; info[4] = g1p_plan_form(plan); info[5] = msm_plan_chain(plan);
  int rc = check_device(device);
  if (rc) return rc;
  DevBuf<int32_t> tabs[G1P_MAX_KEYS], d_terms, part, glv;
  DevBuf<uint8_t> d_flags;
  DevBuf<PlonkKeyDesc> d_desc;
  DevBuf<uint32_t> d_gk;
  for (size_t k = 0; k < n_keys; k++) {
    std::vector<int32_t> pts(n_bases * 2 * BN_NL);
    for (size_t b = 0; b < n_bases; b++) {
      const uint8_t* q = bases + 64 * (k * n_bases + b);
      fp_to_limbs(pts.data() + b * 2 * BN_NL, fp_from_be(q)); fp_to_limbs(pts.data() + b * 2 * BN_NL + BN_NL, fp_from_be(q + 32));
    }
    if ((rc = build_tables_on_device(2, pts, tabs[k]))) return rc;
  }
  const size_t lanes = bn254_g1_msm_scratch_lanes(plan, n);
  if ((rc = d_terms.ensure(ht.size())) || (rc = d_flags.ensure(hf.size())) || (rc = part.ensure((size_t)plan.n_rows * 27 * n)) ||
      (rc = glv.ensure((lanes ? lanes : 1) * (size_t)(G1_GLV_TAB_BYTES_PER_LANE / 4))))
    return rc;
  HIPCK(hipMemcpy(d_terms, ht.data(), ht.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(d_flags, hf.data(), hf.size(), hipMemcpyHostToDevice));
  hipError_t e;
  if (n_keys > 1) {
    // the descriptors of a key set as far as this kernel reads them: the window tables
    std::vector<PlonkKeyDesc> hd(n_keys);
    for (size_t k = 0; k < n_keys; k++) { memset(&hd[k], 0, sizeof hd[k]); hd[k].fixed_tabs = tabs[k]; }
    if ((rc = d_desc.ensure(n_keys)) || (rc = d_gk.ensure(granules))) return rc;
    HIPCK(hipMemcpy(d_desc, hd.data(), n_keys * sizeof(PlonkKeyDesc), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(d_gk, granule_key, granules * sizeof(uint32_t), hipMemcpyHostToDevice));
    e = bn254_launch_g1_msm_rows_keys(plan, d_terms, d_flags, n, (int)n_terms, part, glv, d_desc, (uint32_t)n_keys, d_gk, nullptr);
  } else {
    e = bn254_launch_g1_msm_rows(plan, d_terms, d_flags, n, (int)n_terms, part, glv, tabs[0], nullptr);
  }
  if (e != hipSuccess) return launch_err(e, "probe");
  return g1p_sum_and_fetch(plan, part, n, out_mode, out_points, out_inf, status);
}

int bn254_dbg_g1_sum_rows(const void* rows, int format, int count_a, int count_b, size_t n, int out_mode, uint8_t* out_points, uint8_t* out_inf, uint8_t* status, int device) {
  if (!rows || !out_points || (format & ~1) || (out_mode & ~1) || (out_mode == 0 && !out_inf) || (out_mode == 1 && !status)) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n == 0 || n > (size_t)G1P_MAX_ITEMS) return set_err(BN254_E_BAD_ARG, "bad argument: n is 1 .. 65536");
  if (count_a < 1 || count_b < 0 || count_a > MSM_MAX_ROWS || count_b > MSM_MAX_ROWS || count_a + count_b > MSM_MAX_ROWS) return set_err(BN254_E_BAD_ARG, "bad argument: 1 .. 32 rows in all");
  const size_t n_rows = (size_t)(count_a + count_b);
  // to the kernel's layout: dword (r * 27 + l) * n + i
  std::vector<int32_t> hp(n_rows * 27 * n);
  for (size_t r = 0; r < n_rows; r++)
    for (size_t i = 0; i < n; i++) {
      int32_t d[27];
      if (format) {
        memcpy(d, (const int32_t*)rows + (r * n + i) * 27, sizeof d);
        for (int c = 0; c < 3; c++) if (!g1p_row_digits_ok(d + BN_NL * c)) return set_err(BN254_E_BAD_ARG, "bad argument: digits outside the contract of a row (low digits within 2^28, |value| <= 3 p)");
      } else {
        const uint8_t* q = (const uint8_t*)rows + (r * n + i) * 96;
        for (int c = 0; c < 3; c++) {
          if (!be_lt_p(q + 32 * c)) return set_err(BN254_E_BAD_ARG, "bad argument: a coordinate is not below p");
          fp_to_limbs(d + BN_NL * c, fp_from_be(q + 32 * c));
        }
      }
      for (int l = 0; l < 27; l++) hp[(r * 27 + (size_t)l) * n + i] = d[l];
    }
  MsmPlan plan;
  memset(&plan, 0, sizeof plan);
  plan.n_rows = (int32_t)n_rows; plan.first[0] = 0; plan.count[0] = count_a; plan.first[1] = count_a; plan.count[1] = count_b;
  int rc = check_device(device);
  if (rc) return rc;
  DevBuf<int32_t> part;
  if ((rc = part.ensure(hp.size()))) return rc;
  HIPCK(hipMemcpy(part, hp.data(), hp.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return g1p_sum_and_fetch(plan, part, n, out_mode, out_points, out_inf, status);
}

int bn254_dbg_plonk_group_sums(const uint8_t* p0, const uint8_t* p1, const uint8_t* status, size_t n, uint8_t* out_p0, uint8_t* out_p1, uint8_t* out_group_status,
                               const uint8_t* group_verdicts, uint8_t* status_out, unsigned* n_failed, int device) {
  if (!p0 || !p1 || !status || !out_p0 || !out_p1 || !out_group_status || (group_verdicts && (!status_out || !n_failed))) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (n == 0 || n > (size_t)G1P_MAX_ITEMS) return set_err(BN254_E_BAD_ARG, "bad argument: n is 1 .. 65536");
  if (!g1p_points_canonical(p0, n) || !g1p_points_canonical(p1, n)) return set_err(BN254_E_BAD_ARG, "bad argument: a coordinate is not below p");
  const size_t groups = (n + 63) / 64;
  int rc = check_device(device);
  if (rc) return rc;
  DevBuf<int32_t> ws, gws; DevBuf<uint8_t> st, gst, in, out; DevBuf<uint32_t> fail;
  if ((rc = ws.ensure(n * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = gws.ensure(groups * (size_t)(G16_WS_BYTES_PER_PROOF / 4))) || (rc = st.ensure(n)) || (rc = gst.ensure(groups)) ||
      (rc = in.ensure(128 * n)) || (rc = out.ensure(384 * groups)) || (rc = fail.ensure(1)))
    return rc;
  HIPCK(hipMemset(ws, 0, n * (size_t)G16_WS_BYTES_PER_PROOF));
  HIPCK(hipMemset(gws, 0, groups * (size_t)G16_WS_BYTES_PER_PROOF));
  HIPCK(hipMemset(gst, 0xEE, groups));
  HIPCK(hipMemcpy(in, p0, 64 * n, hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(in + 64 * n, p1, 64 * n, hipMemcpyHostToDevice));
  hipError_t e = bn254_launch_dbg_load(ws, n, st, (int)VE_LX_ELEM, in, 4, nullptr);
  if (e == hipSuccess) e = bn254_launch_dbg_load(ws, n, st, (int)VE_CX_ELEM, in + 64 * n, 4, nullptr);
  if (e != hipSuccess) return launch_err(e, "probe");
  HIPCK(hipMemcpy(st, status, n, hipMemcpyHostToDevice));      // after the loads (same stream): they set PENDING alone
  e = bn254_launch_plonk_group_sums(ws, st, n, gws, gst, VE_LX_ELEM, BN254_ST_LINF, VE_CX_ELEM, BN254_ST_LINF2, nullptr);      // plonk_pass's call
  if (e == hipSuccess) e = bn254_launch_dbg_store(gws, groups, (int)VE_CX_ELEM, out, 0, nullptr);
  if (e != hipSuccess) return launch_err(e, "probe");
  HIPCK(hipDeviceSynchronize());
  std::vector<uint8_t> ho(384 * groups);
  HIPCK(hipMemcpy(ho.data(), out, ho.size(), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(out_group_status, gst, groups, hipMemcpyDeviceToHost));
  for (size_t g = 0; g < groups; g++) { memcpy(out_p0 + 64 * g, ho.data() + 384 * g + 192, 64); memcpy(out_p1 + 64 * g, ho.data() + 384 * g, 64); }
  if (!group_verdicts) return BN254_OK;
  HIPCK(hipMemcpy(gst, group_verdicts, groups, hipMemcpyHostToDevice));
  HIPCK(hipMemset(fail, 0, sizeof(uint32_t)));
  e = bn254_launch_plonk_group_scatter(st, n, gst, fail, nullptr);
  if (e != hipSuccess) return launch_err(e, "probe");
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(status_out, st, n, hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(n_failed, fail, sizeof(uint32_t), hipMemcpyDeviceToHost));
  return BN254_OK;
}

// ---------------------------------------------------------------- the KZG batch (bn254_capi_kzg.hip)
// Part of the library and of a harness that brings bn254_capi_kzg.hip (tests/hostsan/hostsan_kzg.cpp defines BN254_HOSTSAN_KZG); the one-unit host build of
// bn254_capi.hip leaves it out, like the pairing batch
#if defined(__HIPCC__) || defined(BN254_HOSTSAN_KZG)
int bn254_dbg_kzg_fold(const uint8_t* key, const uint8_t* openings, size_t stride, size_t n, const uint8_t* weights, unsigned flags, uint8_t* out_f, uint8_t* out_h,
                       uint8_t* out_inf, uint8_t* out_status, uint8_t* out_group, int device, int form) {
  bool done;
  int rc = kzg_check_args(key, openings, stride, n, out_status, flags, true, &done);
  if (rc) return rc;
  const bool weighted = (flags & BN254_FLAG_RLC) != 0;
  if ((n && (!out_f || !out_h || !out_inf)) || ((weights || out_group) && !weighted)) return set_err(BN254_E_BAD_ARG, "bad argument: weights and out_group need BN254_FLAG_RLC");
  if (device < -1 || form < 0 || form > bn254::PAIRING_FORM_COOP || (form != bn254::PAIRING_FORM_PLAN && device < 0))
    return set_err(BN254_E_BAD_ARG, "bad argument: form 0 runs anywhere, form 1 (lane) and 2 (cooperative) run on a device");
  if (n > (size_t)G1P_MAX_ITEMS || (form == bn254::PAIRING_FORM_COOP && n > (size_t)COOP12_MAX_PROOFS)) return set_err(BN254_E_BAD_ARG, "bad argument: n is at most 65536 (30 720 in the cooperative form)");
  if (done) return BN254_OK;
  KzgProbeHost ph{out_f, out_h, out_inf, out_group};
  if (device < 0) return kzg_fold_on_host(key, openings, stride, n, weights, flags, weighted, ph, out_status);
  return kzg_host_call(key, openings, stride, n, out_status, device, flags, form, weights, weighted, &ph);
}
// ... and of the batch-opening records (bn254_kzg_verify_folded_batch): the same, and out_fold (n x 64 bytes): per record the digest gamma is reduced from and y^ = sum
// gamma^i y_i, canonical (zero for a record the loader decided)
int bn254_dbg_kzg_fold_proof(const uint8_t* key, const uint8_t* records, size_t stride, size_t n, size_t n_digests, size_t data_len, const uint8_t* weights, unsigned flags,
                             uint8_t* out_fold, uint8_t* out_f, uint8_t* out_h, uint8_t* out_inf, uint8_t* out_status, uint8_t* out_group, int device, int form) {
  KzgForm kf;
  bool done;
  int rc = kzg_fold_form(n_digests, data_len, &kf);
  if (rc || (rc = kzg_check_args(key, records, stride, n, out_status, flags, true, &done, kf))) return rc;
  const bool weighted = (flags & BN254_FLAG_RLC) != 0;
  if ((n && (!out_fold || !out_f || !out_h || !out_inf)) || ((weights || out_group) && !weighted)) return set_err(BN254_E_BAD_ARG, "bad argument: weights and out_group need BN254_FLAG_RLC");
  if (device < -1 || form < 0 || form > bn254::PAIRING_FORM_COOP || (form != bn254::PAIRING_FORM_PLAN && device < 0))
    return set_err(BN254_E_BAD_ARG, "bad argument: form 0 runs anywhere, form 1 (lane) and 2 (cooperative) run on a device");
  if (n > (size_t)G1P_MAX_ITEMS || (form == bn254::PAIRING_FORM_COOP && n > (size_t)COOP12_MAX_PROOFS)) return set_err(BN254_E_BAD_ARG, "bad argument: n is at most 65536 (30 720 in the cooperative form)");
  if (done) return BN254_OK;
  KzgProbeHost ph{out_f, out_h, out_inf, out_group, out_fold};
  if (device < 0) return kzg_fold_on_host(key, records, stride, n, weights, flags, weighted, ph, out_status, kf);
  return kzg_host_call(key, records, stride, n, out_status, device, flags, form, weights, weighted, &ph, kf);
}
// whether the G1 walk of n records of n_digests digests plans (both forms must, for every n: what BN254_KZG_FOLD_MAX_DIGESTS is held to); rows: the plan's rows or null
int bn254_dbg_kzg_fold_plan(size_t n_digests, int weighted, size_t n, size_t lane_budget, int joint_g, int* rows) {
  if (n_digests < 1 || n_digests > (size_t)MSM_MAX_FIXED || n == 0) return set_err(BN254_E_BAD_ARG, "bad argument");
  const size_t n_pad = (n + 63) & ~(size_t)63;
  MsmPlan plan;
  if (!msm_plan_build(plan, bn254::kzg_fold_msm_shape((int)n_digests, weighted != 0), n_pad, lane_budget ? lane_budget : msm_lane_budget(), 0, joint_g >= 0 ? joint_g : plonk_joint_g(n_pad)))
    return set_err(BN254_E_BAD_ARG, "shape cannot be planned");
  if (rows) *rows = plan.n_rows;
  return BN254_OK;
}
#endif

// ---------------------------------------------------------------- synthetic workload generator
size_t bn254_synth_groth16_vk_len(size_t n_public) { return 292 + 32 * (n_public + 1) + 4 + 128; }

// the key of the synthetic workload and its trapdoors: the first part of the stream of `seed` (every range and bn254_synth_groth16_for_inputs make the same key)
namespace {
struct SynthKey { U256 alpha, beta, gamma, delta; std::vector<U256> kk; GenTables* tabs; };
GenTables* synth_tables() {   // the window tables of the two generators, built at the first use and shared by the Groth16 and the PlonK generator
  static GenTables* tabs = nullptr;
  static std::mutex tmu;
  std::lock_guard<std::mutex> lk(tmu);
  if (!tabs) { tabs = new GenTables(); build_gen_tables(*tabs); }
  return tabs;
}
void synth_key(uint64_t seed, size_t n_public, int agree, uint8_t* vk_out, SynthKey& key) {
  GenTables* tabs = synth_tables();
  SplitMix64 rng{seed};
  // trapdoors; beta, gamma, delta rejection-sampled into the mode-agreement set when asked:
  // y(beta G2), y(gamma G2) must have c0 / c1 in DIFFERENT halves of [0,p), y(delta G2) in the SAME half
  auto same_half = [](const G2Aff& q) { return fp_is_large(q.y.c0) == fp_is_large(q.y.c1); };
  U256 alpha = fr_random(rng, true), beta, gamma, delta;
  G2Aff beta2, gamma2, delta2;
  const bool agree_modes = (agree & 1) != 0;     // agree bit 1 (value 2): every proof with index = 3 mod 7 has L = the identity (see the worker)
  for (;;) { beta = fr_random(rng, true); beta2 = g2_mul_gen(*tabs, beta); if (!agree_modes || !same_half(beta2)) break; }
  for (;;) { gamma = fr_random(rng, true); gamma2 = g2_mul_gen(*tabs, gamma); if (!agree_modes || !same_half(gamma2)) break; }
  for (;;) { delta = fr_random(rng, true); delta2 = g2_mul_gen(*tabs, delta); if (!agree_modes || same_half(delta2)) break; }
  std::vector<U256> kk(n_public + 1);
  for (auto& k : kk) k = fr_random(rng, true);
  // gnark-compressed vk: alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2 | nK | K.. | 0 (no commitments) | 2 x G2 infinity
  memset(vk_out, 0, bn254_synth_groth16_vk_len(n_public));
  enc_g1_compressed(vk_out, g1_to_affine(g1_mul_gen(*tabs, alpha)));
  enc_g1_compressed(vk_out + 32, g1_to_affine(g1_mul_gen(*tabs, beta)));
  enc_g2_compressed(vk_out + 64, beta2);
  enc_g2_compressed(vk_out + 128, gamma2);
  enc_g1_compressed(vk_out + 192, g1_to_affine(g1_mul_gen(*tabs, delta)));
  enc_g2_compressed(vk_out + 224, delta2);
  uint32_t nk = (uint32_t)(n_public + 1);
  vk_out[288] = (uint8_t)(nk >> 24); vk_out[289] = (uint8_t)(nk >> 16); vk_out[290] = (uint8_t)(nk >> 8); vk_out[291] = (uint8_t)nk;
  for (size_t i = 0; i <= n_public; i++) enc_g1_compressed(vk_out + 292 + 32 * i, g1_to_affine(g1_mul_gen(*tabs, kk[i])));
  size_t off = 292 + 32 * (n_public + 1) + 4;
  vk_out[off] = 0x40; vk_out[off + 64] = 0x40;
  key.alpha = alpha; key.beta = beta; key.gamma = gamma; key.delta = delta; key.kk = kk; key.tabs = tabs;
}
}  // namespace
int bn254_synth_groth16(uint64_t seed, size_t n_public, size_t n, int invalid_every, int agree, int threads, uint8_t* vk_out,
                        uint8_t* proofs_out, uint8_t* inputs_out, uint8_t* expected) {
  return bn254_synth_groth16_range(seed, n_public, 0, n, invalid_every, agree, threads, vk_out, proofs_out, inputs_out, expected);
}
// proofs [first, first + n) of the stream bn254_synth_groth16 generates for `seed` (proof i is a function of (seed, i) alone), written to
// positions 0 .. n-1 of the output buffers: a rank of a sharded job generates its own contiguous shard only
int bn254_synth_groth16_range(uint64_t seed, size_t n_public, size_t first, size_t n, int invalid_every, int agree, int threads, uint8_t* vk_out,
                              uint8_t* proofs_out, uint8_t* inputs_out, uint8_t* expected) {
  if (!vk_out || (n && (!proofs_out || !expected)) || (n && n_public && !inputs_out)) return set_err(BN254_E_BAD_ARG, "bad argument");
  SynthKey key;
  synth_key(seed, n_public, agree, vk_out, key);
  GenTables* tabs = key.tabs;
  const U256 &alpha = key.alpha, &beta = key.beta, &gamma = key.gamma, &delta = key.delta;
  const std::vector<U256>& kk = key.kk;
  if (n == 0) return BN254_OK;
  U256 delta_inv = fr_inv(delta), alpha_beta = fr_mul(alpha, beta);
  // a few twist points outside the r-torsion for the NOT_IN_SUBGROUP class
  std::vector<G2Aff> bad_b;
  if (invalid_every > 0) {
    SplitMix64 r2{seed ^ 0xabcdef1234567ull};
    while (bad_b.size() < 4) {
      G2Aff q; U256 t0 = fr_random(r2, false), t1 = fr_random(r2, false);
      uint8_t b0[32], b1[32]; u256_to_be(b0, t0); u256_to_be(b1, t1);
      q.x.c0 = fp_from_be(b0); q.x.c1 = fp_from_be(b1);
      if (!fp2_sqrt(q.y, fp2_add(fp2_mul(fp2_sqr(q.x), q.x), g2_twist_b()))) continue;
      if (g2_in_subgroup(q)) continue;  // probability ~ 1/cofactor
      bad_b.push_back(q);
    }
  }
  if (threads <= 0) { threads = (int)std::thread::hardware_concurrency(); if (threads <= 0) threads = 1; }
  if ((size_t)threads > n) threads = (int)n;
  G1Aff g1gen; g1gen.x = fp_one(); g1gen.y = fp_add(fp_one(), fp_one());
  auto worker = [&](int tid) {
    for (size_t li = tid; li < n; li += threads) {
      const size_t i = first + li;   // global index: seeds the proof and selects its class
      SplitMix64 r{seed * 0x9e3779b97f4a7c15ull + 0x1000 + i};
      U256 a = fr_random(r, true), b = fr_random(r, true);
      U256 ell = kk[0];
      std::vector<U256> xs(n_public);
      for (size_t s = 0; s < n_public; s++) { xs[s] = fr_random(r, false); ell = fr_add(ell, fr_mul(xs[s], kk[s + 1])); }
      if ((agree & 2) && n_public > 0 && i % 7 == 3) {
        // L = K0 + sum x_s K_s = the identity: the last input cancels the rest (valid proofs whose public-input point is the point at infinity --
        // bn::pairing_batch skips such a pair; the kernels replace its line by 1)
        const size_t last = n_public - 1;
        ell = fr_sub(ell, fr_mul(xs[last], kk[last + 1]));
        U256 zero = {{0, 0, 0, 0}};
        xs[last] = fr_mul(fr_sub(zero, ell), fr_inv(kk[last + 1]));
        ell = zero;
      }
      // c = (a b - alpha beta - gamma ell) / delta   =>   e(A,B) = e(alpha,beta) e(L,gamma) e(C,delta)
      U256 c = fr_mul(fr_sub(fr_sub(fr_mul(a, b), alpha_beta), fr_mul(gamma, ell)), delta_inv);
      G1Aff A = g1_to_affine(g1_mul_gen(*tabs, a));
      G2Aff B = g2_mul_gen(*tabs, b);
      G1Proj Cp = g1_mul_gen(*tabs, c);
      uint8_t st = BN254_ACCEPT;
      int cls = -1;
      if (invalid_every > 0 && (i % (size_t)invalid_every) == (size_t)invalid_every - 1) cls = (int)((i / (size_t)invalid_every) % 5);
      if (cls == 1) { Cp = g1_add_mixed(Cp, g1gen); st = BN254_REJECT; }
      if (cls == 3) { B = bad_b[(i / (size_t)invalid_every) % bad_b.size()]; st = BN254_ERR_NOT_IN_SUBGROUP; }
      G1Aff C = g1_is_identity(Cp) ? g1gen : g1_to_affine(Cp);
      uint8_t* p = proofs_out + 256 * li;
      enc_g1_uncompressed(p, A); enc_g2_uncompressed(p + 64, B); enc_g1_uncompressed(p + 192, C);
      for (size_t s = 0; s < n_public; s++) u256_to_be(inputs_out + (li * n_public + s) * 32, xs[s]);
      if (cls == 0 && n_public > 0) {  // x_0 + 1 (as raw integer; stays below 2^256)
        U256 one = {{1, 0, 0, 0}}, t; u256_add(t, xs[0], one); u256_to_be(inputs_out + li * n_public * 32, t); st = BN254_REJECT;
      }
      if (cls == 2) {  // A.y + 1 mod p: off the curve (y+1 = -y only for y = (p-1)/2)
        Fp y1 = fp_add(A.y, fp_one()); fp_to_be(p + 32, y1); st = BN254_ERR_NOT_ON_CURVE;
      }
      if (cls == 4) { memset(p, 0xff, 32); st = BN254_ERR_NOT_MEMBER; }  // A.x = 2^256 - 1 >= p
      expected[li] = st;
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++) th.emplace_back(worker, t);
  for (auto& x : th) x.join();
  return BN254_OK;
}

// valid proofs for given public inputs under the key of bn254_synth_groth16(seed, n_public, .., agree = 1): A = a G1, B = b G2, C = (a b - alpha beta - gamma ell) / delta G1
// with ell = k_0 + sum (x_s mod r) k_s (the trapdoor formula of the generator above); a, b from (seed, i) like the generator's proof i
int bn254_synth_groth16_for_inputs(uint64_t seed, size_t n_public, size_t n, const uint8_t* inputs, int threads, uint8_t* vk_out, uint8_t* proofs_out) {
  if (!vk_out || (n && !proofs_out) || (n && n_public && !inputs)) return set_err(BN254_E_BAD_ARG, "bad argument");
  SynthKey key;
  synth_key(seed, n_public, 1, vk_out, key);
  if (n == 0) return BN254_OK;
  const U256 delta_inv = fr_inv(key.delta), alpha_beta = fr_mul(key.alpha, key.beta), r = u256_r();
  if (threads <= 0) { threads = (int)std::thread::hardware_concurrency(); if (threads <= 0) threads = 1; }
  if ((size_t)threads > n) threads = (int)n;
  auto worker = [&](int tid) {
    for (size_t i = tid; i < n; i += threads) {
      SplitMix64 g{seed * 0x9e3779b97f4a7c15ull + 0x1000 + i};
      const U256 a = fr_random(g, true), b = fr_random(g, true);
      U256 ell = key.kk[0];
      for (size_t s = 0; s < n_public; s++) {
        const uint8_t* q = inputs + (i * n_public + s) * 32;
        U256 x;
        for (int l = 0; l < 4; l++) { x.l[l] = 0; for (int j = 0; j < 8; j++) x.l[l] = x.l[l] << 8 | q[(3 - l) * 8 + j]; }
        while (u256_cmp(x, r) >= 0) u256_sub(x, x, r);   // 2^256 < 6 r
        ell = fr_add(ell, fr_mul(x, key.kk[s + 1]));
      }
      const U256 c = fr_mul(fr_sub(fr_sub(fr_mul(a, b), alpha_beta), fr_mul(key.gamma, ell)), delta_inv);
      uint8_t* p = proofs_out + 256 * i;
      enc_g1_uncompressed(p, g1_to_affine(g1_mul_gen(*key.tabs, a)));
      enc_g2_uncompressed(p + 64, g2_mul_gen(*key.tabs, b));
      const G1Proj cp = g1_mul_gen(*key.tabs, c);
      if (g1_is_identity(cp)) { memset(p + 192, 0, 64); } else enc_g1_uncompressed(p + 192, g1_to_affine(cp));
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++) th.emplace_back(worker, t);
  for (auto& x : th) x.join();
  return BN254_OK;
}

// ---------------------------------------------------------------- synthetic PlonK workload generator
// Valid proofs for a key of any shape, from the KZG secret: a simulator that knows tau and the discrete logarithm of every commitment can open any
// commitment to any value, so it draws the commitments and the claimed values at random, derives the challenges as the verifier does, sets the one
// value the verifier recomputes (the opening of the linearised polynomial's constant term) and solves the two KZG quotients.
// The formulas below restate plonk/verify.rs:97-284 and kzg.rs:46-72 over scalars; only Challenge and bsb22_hash_to_field are the verifier's own code.
// Whether a proof made here passes is decided by the oracle (tests/test_plonk_synth_cpu.py), not by this file.
size_t bn254_synth_plonk_vk_len(size_t n_qcp) { return 34328 + 40 * n_qcp; }
size_t bn254_synth_plonk_proof_len(size_t n_qcp) { return 808 + 96 * n_qcp; }

namespace {
enum { SP_L = 0, SP_R, SP_O, SP_Z, SP_H0, SP_H1, SP_H2, SP_BSB0, SP_MAX_PTS = SP_BSB0 + PLONK_MAX_QCP };
enum { SK_S1 = 0, SK_S2, SK_S3, SK_QL, SK_QR, SK_QM, SK_QO, SK_QK, SK_QCP0 };       // the order of the key's points in its bytes and in PlonkKey::enc
struct SynthPlonkKey { PlonkKey vk; FrM tau; FrM k[SK_QCP0 + PLONK_MAX_QCP]; GenTables* tabs; size_t n_public; int n_qcp; };
inline FrM frm_of(const U256& u) { const FrM c = {{u.l[0], u.l[1], u.l[2], u.l[3]}}; return fr_ctx().from_canon(c); }
inline U256 u256_of(const FrM& a) { const FrM c = fr_ctx().to_canon(a); const U256 u = {{c.l[0], c.l[1], c.l[2], c.l[3]}}; return u; }
inline FrM frm_random(SplitMix64& g, bool nonzero) { return frm_of(fr_random(g, nonzero)); }
inline void put_be64(uint8_t* b, uint64_t v) { for (int j = 0; j < 8; j++) b[j] = (uint8_t)(v >> (56 - 8 * j)); }
inline void put_be32(uint8_t* b, uint32_t v) { for (int j = 0; j < 4; j++) b[j] = (uint8_t)(v >> (24 - 8 * j)); }
inline void put_g1_mul(uint8_t* out64, const GenTables& t, const FrM& k) {           // k G uncompressed; the identity as 64 zero bytes
  const G1Proj p = g1_mul_gen(t, u256_of(k));
  if (g1_is_identity(p)) memset(out64, 0, 64); else enc_g1_uncompressed(out64, g1_to_affine(p));
}
int synth_plonk_args(size_t n_public, size_t n_qcp, unsigned log2_size, size_t n, size_t proof_stride, const void* vk_out, const void* proofs_out) {
  if (n_qcp > (size_t)PLONK_MAX_QCP || log2_size < 1 || log2_size > 28) return set_err(BN254_E_BAD_ARG, "bad argument: at most 8 commitments, log2_size in 1..28");
  const size_t size = (size_t)1 << log2_size;
  if (n_public > size || n_qcp > size - n_public) return set_err(BN254_E_BAD_ARG, "bad argument: the domain is smaller than n_public + n_qcp");
  if (proof_stride < bn254_synth_plonk_proof_len(n_qcp)) return set_err(BN254_E_BAD_ARG, "bad argument: proof_stride below the proof length");
  if (!vk_out || (n && !proofs_out)) return set_err(BN254_E_BAD_ARG, "bad argument");
  return BN254_OK;
}
// the key of (seed, n_public, n_qcp, log2_size) and its trapdoors.  Arguments checked by the caller.
void synth_plonk_key(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, uint8_t* vk_out, SynthPlonkKey& key) {
  const FrCtx& F = fr_ctx();
  GenTables* tabs = synth_tables();
  SplitMix64 rng{(seed ^ 0x504c4f4e4b5f564bull) + 0x9e3779b97f4a7c15ull * ((uint64_t)n_public * 0x100000001b3ull + (uint64_t)n_qcp * 64 + log2_size)};
  const uint64_t size = (uint64_t)1 << log2_size;
  uint8_t* b = vk_out;
  memset(b, 0, bn254_synth_plonk_vk_len(n_qcp));
  // the domain: omega = x^((r - 1) / size) of exact order size (r - 1 = 2^28 * odd)
  U256 e = u256_r(); e.l[0] -= 1;
  for (unsigned s = 0; s < log2_size; s++) { for (int i = 0; i < 3; i++) e.l[i] = (e.l[i] >> 1) | (e.l[i + 1] << 63); e.l[3] >>= 1; }
  FrM omega;
  for (;;) {
    const FrM x = frm_random(rng, true);
    omega = F.one;
    for (int i = 255; i >= 0; i--) { omega = F.mul(omega, omega); if ((e.l[i >> 6] >> (i & 63)) & 1) omega = F.mul(omega, x); }
    if (!F.eq(F.pow_u64(omega, size >> 1), F.one)) break;
  }
  const FrM coset = frm_random(rng, true);
  put_be64(b, size); F.to_be(b + 8, F.inverse(F.from_u64(size))); F.to_be(b + 40, omega); put_be64(b + 72, (uint64_t)n_public); F.to_be(b + 80, coset);
  key.tau = frm_random(rng, true);
  for (size_t i = 0; i < SK_QCP0 + n_qcp; i++) key.k[i] = frm_random(rng, true);
  for (int i = 0; i < 8; i++) enc_g1_compressed(b + 112 + 32 * i, g1_to_affine(g1_mul_gen(*tabs, u256_of(key.k[i]))));
  put_be32(b + 368, (uint32_t)n_qcp);
  size_t off = 372;
  for (size_t i = 0; i < n_qcp; i++, off += 32) enc_g1_compressed(b + off, g1_to_affine(g1_mul_gen(*tabs, u256_of(key.k[SK_QCP0 + i]))));
  G1Aff g1gen; g1gen.x = fp_one(); g1gen.y = fp_add(fp_one(), fp_one());
  enc_g1_compressed(b + off, g1gen);
  // g2 = [sigma G2, sigma tau G2], re-sampled until both compressed points decode back to themselves in the loader's reading of the root order (parse_plonk_vk)
  for (;;) {
    const FrM sigma = frm_random(rng, true);
    const G2Aff q[2] = {g2_mul_gen(*tabs, u256_of(sigma)), g2_mul_gen(*tabs, u256_of(F.mul(sigma, key.tau)))};
    bool same = true;
    for (int j = 0; j < 2 && same; j++) {
      uint8_t want[128], got[128]; G2Aff back;
      enc_g2_compressed(b + off + 32 + 64 * j, q[j]);
      same = dec_g2_compressed(back, b + off + 32 + 64 * j, 0) == DEC_OK;
      if (same) { enc_g2_uncompressed(want, q[j]); enc_g2_uncompressed(got, back); same = memcmp(want, got, 128) == 0; }
    }
    if (same) break;
    key.tau = frm_random(rng, true);
  }
  off += 160 + 33788;            // the precomputed lines the loader skips: zeros
  put_be64(b + off, (uint64_t)n_qcp); off += 8;
  // the commitment constraints: n_qcp distinct ascending rows of [0, size - n_public)
  uint64_t cci[PLONK_MAX_QCP];
  const uint64_t range = size - (uint64_t)n_public;
  for (size_t i = 0; i < n_qcp;) {
    const uint64_t v = rng.next() % range;
    bool fresh = true;
    for (size_t j = 0; j < i; j++) fresh = fresh && cci[j] != v;
    if (fresh) cci[i++] = v;
  }
  std::sort(cci, cci + n_qcp);
  for (size_t i = 0; i < n_qcp; i++, off += 8) put_be64(b + off, cci[i]);
  (void)parse_plonk_vk(key.vk, b, off);       // the loader's own image of the bytes: encodings, transcript prefix, omega^(n_public + cci)
  key.tabs = tabs; key.n_public = n_public; key.n_qcp = (int)n_qcp;
}
// One proof for the input row `in` (n_public canonical values), randomness from g; cls: -1 valid, 1..5 the corruption classes that touch the proof (class 0 touches
// the inputs: the caller's).  p: proof_len bytes, zeroed.
void synth_plonk_proof(const SynthPlonkKey& key, SplitMix64& g, const uint8_t* in, int cls, uint8_t* p) {
  const FrCtx& F = fr_ctx();
  const PlonkKey& vk = key.vk;
  const GenTables& tabs = *key.tabs;
  const int q = key.n_qcp, nd = 6 + q, npts = SP_BSB0 + q;
  const size_t off_claimed = 516, off_zs = off_claimed + 32 * (size_t)nd, off_bsb = off_zs + 100;
  // 1. the commitments: known multiples of G
  FrM d[SP_MAX_PTS]; G1Proj pj[SP_MAX_PTS]; G1Aff pa[SP_MAX_PTS];
  for (int k = 0; k < npts; k++) { d[k] = frm_random(g, true); pj[k] = g1_mul_gen(tabs, u256_of(d[k])); }
  g1_batch_to_affine(pa, pj, (size_t)npts);
  for (int k = 0; k < SP_BSB0; k++) enc_g1_uncompressed(p + 64 * k, pa[k]);
  for (int j = 0; j < q; j++) enc_g1_uncompressed(p + off_bsb + 64 * j, pa[SP_BSB0 + j]);
  put_be32(p + 512, (uint32_t)nd); put_be32(p + off_zs + 96, (uint32_t)q);
  // 2. gamma, beta, alpha, zeta (verify.rs:62-95)
  uint8_t dg[32], db[32], da[32], dz[32];
  Challenge cg(vk.gamma_mid); cg.bind(in, 32 * key.n_public); cg.bind(p, 192);
  const FrM gamma = cg.finish(dg);
  Challenge cb("beta", 4, dg);
  const FrM beta = cb.finish(db);
  Challenge ca("alpha", 5, db); ca.bind(p + off_bsb, 64 * (size_t)q); ca.bind(p + 192, 64);
  const FrM alpha = ca.finish(da);
  Challenge cz("zeta", 4, da); cz.bind(p + 256, 192);
  const FrM zeta = cz.finish(dz);
  // 3. the claimed values at random, but the first: the constant term of the linearised polynomial as verify.rs:97-207 computes it
  FrM cl[PLONK_MAX_CLAIMED];
  for (int k = 1; k < nd; k++) cl[k] = frm_random(g, false);
  const FrM zu = frm_random(g, false);
  const FrM &l = cl[1], &r = cl[2], &o = cl[3], &s1 = cl[4], &s2 = cl[5];
  const FrM zeta_n = F.pow_u64(zeta, vk.size), zh = F.sub(zeta_n, F.one), zs = F.mul(zh, vk.size_inv);
  const FrM lagrange_one = F.mul(zs, F.inverse(F.sub(zeta, F.one)));
  FrM pi = {{0, 0, 0, 0}}, accw = F.one;
  for (size_t i = 0; i < key.n_public; i++) {
    pi = F.add(pi, F.mul(F.mul(F.mul(zs, F.inverse(F.sub(zeta, accw))), accw), F.from_be32(in + 32 * i)));
    accw = F.mul(accw, vk.generator);
  }
  for (int j = 0; j < q; j++) pi = F.add(pi, F.mul(F.mul(F.mul(zs, vk.wpow[j]), F.inverse(F.sub(zeta, vk.wpow[j]))), bsb22_hash_to_field(p + off_bsb + 64 * j)));
  const FrM a2l1 = F.mul(F.mul(lagrange_one, alpha), alpha);
  const FrM bs1 = F.add(F.add(F.mul(beta, s1), gamma), l), bs2 = F.add(F.add(F.mul(beta, s2), gamma), r);
  cl[0] = F.neg(F.add(F.sub(F.mul(F.mul(F.mul(F.mul(bs1, bs2), F.add(o, gamma)), alpha), zu), a2l1), pi));
  // 4. the linearised digest's discrete logarithm: the combination of verify.rs:216-284 over scalars
  const FrM c_s3 = F.mul(F.mul(F.mul(F.mul(bs1, bs2), beta), alpha), zu);
  const FrM u = F.mul(beta, vk.coset_shift), u2 = F.mul(u, vk.coset_shift);
  FrM t = F.add(F.add(F.mul(beta, zeta), gamma), l);
  t = F.mul(t, F.add(F.add(F.mul(u, zeta), gamma), r));
  t = F.mul(t, F.add(F.add(F.mul(u2, zeta), gamma), o));
  const FrM c_z = F.sub(a2l1, F.mul(t, alpha));
  const FrM zn2 = F.mul(zeta_n, F.mul(zeta, zeta));
  FrM lin = F.mul(key.k[SK_QL], l);
  lin = F.add(lin, F.mul(key.k[SK_QR], r));
  lin = F.add(lin, F.mul(key.k[SK_QM], F.mul(l, r)));
  lin = F.add(lin, F.mul(key.k[SK_QO], o));
  lin = F.add(lin, key.k[SK_QK]);
  lin = F.add(lin, F.mul(key.k[SK_S3], c_s3));
  lin = F.add(lin, F.mul(d[SP_Z], c_z));
  lin = F.sub(lin, F.mul(zh, F.add(d[SP_H0], F.mul(zn2, F.add(d[SP_H1], F.mul(zn2, d[SP_H2]))))));
  for (int j = 0; j < q; j++) lin = F.add(lin, F.mul(d[SP_BSB0 + j], cl[6 + j]));
  for (int k = 0; k < nd; k++) F.to_be(p + off_claimed + 32 * k, cl[k]);
  F.to_be(p + off_zs + 64, zu);
  // 5. the folding challenge (kzg.rs:46-72) and the two quotients
  uint8_t b32[32], lin_enc[64], dgam[32];
  put_g1_mul(lin_enc, tabs, lin);
  Challenge cf("gamma", 5, nullptr);
  F.to_be(b32, zeta); cf.bind(b32, 32);
  cf.bind(lin_enc, 64); cf.bind(p, 192); cf.bind(vk.enc[SK_S1], 64); cf.bind(vk.enc[SK_S2], 64);
  for (int j = 0; j < q; j++) cf.bind(vk.enc[SK_QCP0 + j], 64);
  cf.bind(p + off_claimed, 32 * (size_t)nd); cf.bind(p + off_zs + 64, 32);
  const FrM fold = cf.finish(dgam);
  FrM dig[PLONK_MAX_CLAIMED] = {lin, d[SP_L], d[SP_R], d[SP_O], key.k[SK_S1], key.k[SK_S2]};
  for (int j = 0; j < q; j++) dig[6 + j] = key.k[SK_QCP0 + j];
  FrM num = {{0, 0, 0, 0}}, gk = F.one;
  for (int k = 0; k < nd; k++) { num = F.add(num, F.mul(gk, F.sub(dig[k], cl[k]))); gk = F.mul(gk, fold); }
  const FrM h = F.mul(num, F.inverse(F.sub(key.tau, zeta)));
  FrM hs = F.mul(F.sub(d[SP_Z], zu), F.inverse(F.sub(key.tau, F.mul(zeta, vk.generator))));
  if (cls == 1) hs = F.add(hs, F.one);                                                   // H' + G
  put_g1_mul(p + 448, tabs, h);
  put_g1_mul(p + off_zs, tabs, hs);
  // the corruptions of a finished proof
  if (cls == 2) fp_to_be(p + 32, fp_add(pa[SP_L].y, fp_one()));                           // L.y + 1 mod p
  if (cls == 3) memset(p + 192, 0xff, 32);                                                // Z.x = 2^256 - 1
  if (cls == 4) F.to_be(p + off_claimed + 32 * 6, F.add(cl[6], F.one));                   // the first commitment's selector claim + 1
  if (cls == 5) { put_be32(p + off_zs + 96, (uint32_t)(q - 1)); memset(p + off_bsb + 64 * (size_t)(q - 1), 0, 64); }   // the last commitment dropped
}
int synth_plonk_run(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, size_t first, size_t n, int invalid_every, const uint8_t* given, int threads,
                    uint8_t* vk_out, uint8_t* proofs_out, size_t proof_stride, uint8_t* inputs_out, uint8_t* expected) {
  SynthPlonkKey key;
  synth_plonk_key(seed, n_public, n_qcp, log2_size, vk_out, key);
  if (n == 0) return BN254_OK;
  const FrCtx& F = fr_ctx();
  static const uint8_t none = 0;
  if (threads <= 0) { threads = (int)std::thread::hardware_concurrency(); if (threads <= 0) threads = 1; }
  if ((size_t)threads > n) threads = (int)n;
  auto worker = [&](int tid) {
    for (size_t li = tid; li < n; li += threads) {
      const size_t i = first + li;     // global index: seeds the proof and selects its class
      SplitMix64 g{seed * 0x9e3779b97f4a7c15ull + 0x2000 + i};
      uint8_t* p = proofs_out + proof_stride * li;
      memset(p, 0, proof_stride);
      const uint8_t* in = !n_public ? &none : given ? given + li * n_public * 32 : inputs_out + li * n_public * 32;
      if (!given) for (size_t s = 0; s < n_public; s++) u256_to_be(inputs_out + (li * n_public + s) * 32, fr_random(g, false));
      int cls = -1;
      if (!given && invalid_every > 0 && (i % (size_t)invalid_every) == (size_t)invalid_every - 1) cls = (int)((i / (size_t)invalid_every) % 6);
      if ((cls == 0 && n_public == 0) || ((cls == 4 || cls == 5) && n_qcp == 0)) cls = 1;
      synth_plonk_proof(key, g, in, cls, p);
      if (cls == 0) F.to_be(inputs_out + li * n_public * 32, F.add(F.from_be32(in), F.one));   // public input 0 + 1 mod r
      if (expected) {
        static const uint8_t st[6] = {BN254_ERR_OPENING_MISMATCH, BN254_ERR_PAIRING_FAILED, BN254_ERR_NOT_ON_CURVE, BN254_ERR_NOT_MEMBER, BN254_ERR_PAIRING_FAILED, BN254_ERR_BSB22_MISMATCH};
        expected[li] = cls < 0 ? (uint8_t)BN254_ACCEPT : st[cls];
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++) th.emplace_back(worker, t);
  for (auto& x : th) x.join();
  return BN254_OK;
}
}  // namespace
int bn254_synth_plonk(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, size_t n, int invalid_every, int threads, uint8_t* vk_out, uint8_t* proofs_out,
                      size_t proof_stride, uint8_t* inputs_out, uint8_t* expected) {
  return bn254_synth_plonk_range(seed, n_public, n_qcp, log2_size, 0, n, invalid_every, threads, vk_out, proofs_out, proof_stride, inputs_out, expected);
}
// proofs [first, first + n) of the stream of bn254_synth_plonk (proof i is a function of (seed, i) and the key alone), written to positions 0 .. n-1
int bn254_synth_plonk_range(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, size_t first, size_t n, int invalid_every, int threads, uint8_t* vk_out,
                            uint8_t* proofs_out, size_t proof_stride, uint8_t* inputs_out, uint8_t* expected) {
  int rc = synth_plonk_args(n_public, n_qcp, log2_size, n, proof_stride, vk_out, proofs_out);
  if (rc) return rc;
  if (n && (!expected || (n_public && !inputs_out))) return set_err(BN254_E_BAD_ARG, "bad argument");
  return synth_plonk_run(seed, n_public, n_qcp, log2_size, first, n, invalid_every, nullptr, threads, vk_out, proofs_out, proof_stride, inputs_out, expected);
}
// the key of bn254_synth_plonk for the same arguments and one valid proof per given input row (n x n_public x 32 bytes, big-endian, each below r)
int bn254_synth_plonk_for_inputs(uint64_t seed, size_t n_public, size_t n_qcp, unsigned log2_size, size_t n, const uint8_t* inputs, int threads, uint8_t* vk_out,
                                 uint8_t* proofs_out, size_t proof_stride) {
  int rc = synth_plonk_args(n_public, n_qcp, log2_size, n, proof_stride, vk_out, proofs_out);
  if (rc) return rc;
  if (n && n_public && !inputs) return set_err(BN254_E_BAD_ARG, "bad argument");
  const U256 r = u256_r();
  for (size_t k = 0; k < n * n_public; k++) {
    U256 x;
    for (int l = 0; l < 4; l++) x.l[l] = be64(inputs + 32 * k + (3 - l) * 8);
    if (u256_cmp(x, r) >= 0) return set_err(BN254_E_BAD_ARG, "bad argument: a public input is not below r");
  }
  static const uint8_t none = 0;     // `given` non-null selects the caller's rows
  return synth_plonk_run(seed, n_public, n_qcp, log2_size, 0, n, 0, n_public ? inputs : &none, threads, vk_out, proofs_out, proof_stride, nullptr, nullptr);
}

}  // extern "C"
