// bn254_capi_vkbatch.hip -- bn254_groth16_vk_prepare_batch: many Groth16 verifying keys prepared in one call, on the device.  The host scans the structure of every
// key (bn254_host.hpp::scan_g16_vk, the walk the single-key path makes), gathers the compressed points of a pass into pinned memory, launches the kernels of
// bn254_k_vkprep.hip and the one-pair pairing program, and fills one G16Prepared per key that loaded from what comes back.  No key's per-device state is touched and no
// K-point table is built: both stay lazy, as for a handle of bn254_groth16_vk_prepare.
// A call works through its list in passes of at most VKP_PASS_KEYS keys and VKP_PASS_G1 compressed G1 points (a key with more points than that is a pass of its own),
// so its device scratch is bounded whatever n_keys is: 2 x 19 008 bytes of line tables and 4680 bytes of pairing workspace per key, 176 MB at 4096 keys, plus 104 bytes
// per G1 point.  BN254_VKPREP_PASS (tests; read once) lowers the keys per pass.
// Not part of the one-translation-unit host build of bn254_capi.hip (tests/hostsan/hostsan_main.cpp): a harness that wants it includes this file itself.
#include "bn254_capi_internal.h"
#include "bn254_vkprep.h"

#define VKP_PASS_KEYS 4096
#define VKP_PASS_G1 ((size_t)1 << 18)

static const size_t g_vkp_pass_keys = [] { long v = env_long("BN254_VKPREP_PASS", VKP_PASS_KEYS); return (size_t)(v < 1 ? 1 : (v > VKP_PASS_KEYS ? VKP_PASS_KEYS : v)); }();

namespace {

// one pass on the host's side: what goes to the lanes and what comes back
struct VkpPass {
  std::vector<size_t> key_of;                 // position in the call's list
  std::vector<bn254::VkpKey> keys;
  std::vector<uint32_t> g1_src, g2_src;
  size_t n_g1 = 0;
  // results (pointers into pinned memory after a device pass, into `own` after a host pass)
  const int32_t *g1pts = nullptr, *barg = nullptr, *tabs = nullptr;
  const uint8_t *key_ok = nullptr, *tab_ok = nullptr, *gt = nullptr;
  std::vector<int32_t> own_i; std::vector<uint8_t> own_b;
  void clear() { key_of.clear(); keys.clear(); g1_src.clear(); g2_src.clear(); n_g1 = 0; }
};

void vkp_add_key(VkpPass& p, size_t pos, const uint8_t* vk, const G16VkLayout& l) {
  const size_t g1 = p.g1_src.size(), g2 = p.g2_src.size();
  p.g1_src.resize(g1 + 8 * (VKP_G1_FIXED + (size_t)l.nk));
  p.g2_src.resize(g2 + 16 * VKP_G2_PER_KEY);
  uint8_t* d1 = (uint8_t*)(p.g1_src.data() + g1);
  memcpy(d1, vk + G16_VK_ALPHA, 32); memcpy(d1 + 32, vk + G16_VK_BETA1, 32); memcpy(d1 + 64, vk + G16_VK_DELTA1, 32);
  if (l.nk) memcpy(d1 + 96, vk + l.k_off, 32 * (size_t)l.nk);
  uint8_t* d2 = (uint8_t*)(p.g2_src.data() + g2);
  memcpy(d2, vk + G16_VK_BETA, 64); memcpy(d2 + 64, vk + G16_VK_GAMMA, 64); memcpy(d2 + 128, vk + G16_VK_DELTA, 64); memcpy(d2 + 192, vk + l.ck_off, 128);
  p.keys.push_back(bn254::VkpKey{(uint32_t)p.n_g1, (uint32_t)(VKP_G1_FIXED + l.nk)});
  p.key_of.push_back(pos);
  p.n_g1 += VKP_G1_FIXED + (size_t)l.nk;
}

// dword counts of the results of a pass of m keys and n_g1 points, in the order they lie in one buffer: g1pts | barg | tabs, then the bytes key_ok | tab_ok | gt
struct VkpSizes {
  size_t g1pts, barg, tabs, key_ok, tab_ok, gt;
  VkpSizes(size_t m, size_t n_g1) : g1pts(n_g1 * VKP_G1_DWORDS), barg(m * VKP_G2_DWORDS), tabs(2 * m * (size_t)VKP_TAB_DWORDS), key_ok(m), tab_ok(2 * m), gt(m * 384) {}
  size_t dwords() const { return g1pts + barg + tabs; }
  size_t bytes() const { return key_ok + tab_ok + gt; }
};

// the lane bodies on the host, one after the other (bn254_dbg_g16_vk_prepare_batch with device -1)
void vkp_run_host(VkpPass& p, int mode) {
  const size_t m = p.keys.size(), n_g2 = m * VKP_G2_PER_KEY;
  const VkpSizes z(m, p.n_g1);
  p.own_i.assign(z.dwords(), 0); p.own_b.assign(z.bytes(), 0);
  std::vector<uint8_t> ok(p.n_g1 + n_g2), pair(m * 192);
  std::vector<int32_t> g2pts(n_g2 * VKP_G2_DWORDS), targ(2 * m * VKP_G2_DWORDS);
  VkpLaunchArgs a;
  a.m = (uint32_t)m; a.n_g1 = (uint32_t)p.n_g1; a.mode = mode;
  a.g1_src = p.g1_src.data(); a.g2_src = p.g2_src.data(); a.keys = p.keys.data();
  a.g1pts = p.own_i.data(); a.barg = a.g1pts + z.g1pts; a.tabs = a.barg + z.barg;
  a.ok1 = ok.data(); a.ok2 = ok.data() + p.n_g1;
  a.g2pts = g2pts.data(); a.targ = targ.data();
  a.key_ok = p.own_b.data(); a.tab_ok = a.key_ok + z.key_ok; a.gt = a.tab_ok + z.tab_ok;
  a.pair_g1 = pair.data(); a.pair_g2 = pair.data() + m * 64;
  a.ws = nullptr; a.ws_status = nullptr;
  vkp_run_on_host(a);
  p.g1pts = a.g1pts; p.barg = a.barg; p.tabs = a.tabs; p.key_ok = a.key_ok; p.tab_ok = a.tab_ok; p.gt = a.gt;
}

// the device buffers, the pinned staging and the stream of one call; sized by the first pass that needs more
struct VkpDev {
  Stream stream;
  Event ev[VKP_NUM_EVENTS]; bool timed = false;
  DevBuf<uint32_t> d_src; DevBuf<bn254::VkpKey> d_keys;
  DevBuf<int32_t> d_out, d_g2pts, d_targ, d_ws;
  DevBuf<uint8_t> d_bytes, d_ok, d_pair, d_ws_status;
  PinBuf<uint32_t> h_src; PinBuf<bn254::VkpKey> h_keys; PinBuf<int32_t> h_out; PinBuf<uint8_t> h_bytes;
};

int vkp_run_device(VkpPass& p, int mode, VkpDev& d, float* stage_ms) {
  const size_t m = p.keys.size(), n_g2 = m * VKP_G2_PER_KEY;
  const VkpSizes z(m, p.n_g1);
  const int oom = BN254_E_NOMEM;
  int rc;
  if ((rc = d.stream.ensure())) return rc;
  if (stage_ms && !d.timed) { for (auto& e : d.ev) if ((rc = e.ensure_timed())) return rc; d.timed = true; }
  const size_t src_dw = p.g1_src.size() + p.g2_src.size();
  if ((rc = d.h_src.ensure(src_dw)) || (rc = d.h_keys.ensure(m)) || (rc = d.h_out.ensure(z.dwords())) || (rc = d.h_bytes.ensure(z.bytes())) ||
      (rc = d.d_src.ensure(src_dw, oom)) || (rc = d.d_keys.ensure(m, oom)) || (rc = d.d_out.ensure(z.dwords(), oom)) || (rc = d.d_g2pts.ensure(n_g2 * VKP_G2_DWORDS, oom)) ||
      (rc = d.d_targ.ensure(2 * m * VKP_G2_DWORDS, oom)) || (rc = d.d_ws.ensure(m * (size_t)(G16_WS_BYTES_PER_PROOF / 4), oom)) || (rc = d.d_bytes.ensure(z.bytes(), oom)) ||
      (rc = d.d_ok.ensure(p.n_g1 + n_g2, oom)) || (rc = d.d_pair.ensure(m * 192, oom)) || (rc = d.d_ws_status.ensure(m, oom)))
    return rc;
  memcpy(d.h_src, p.g1_src.data(), p.g1_src.size() * 4);
  memcpy(d.h_src + p.g1_src.size(), p.g2_src.data(), p.g2_src.size() * 4);
  memcpy(d.h_keys, p.keys.data(), m * sizeof(bn254::VkpKey));
  hipStream_t s = d.stream;
  HIPCK(hipMemcpyAsync(d.d_src, d.h_src, src_dw * 4, hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(d.d_keys, d.h_keys, m * sizeof(bn254::VkpKey), hipMemcpyHostToDevice, s));
  VkpLaunchArgs a;
  a.m = (uint32_t)m; a.n_g1 = (uint32_t)p.n_g1; a.mode = mode;
  a.g1_src = d.d_src; a.g2_src = d.d_src + p.g1_src.size(); a.keys = d.d_keys;
  a.g1pts = d.d_out; a.barg = d.d_out + z.g1pts; a.tabs = d.d_out + z.g1pts + z.barg;
  a.ok1 = d.d_ok; a.ok2 = d.d_ok + p.n_g1;
  a.g2pts = d.d_g2pts; a.targ = d.d_targ;
  a.key_ok = d.d_bytes; a.tab_ok = d.d_bytes + z.key_ok; a.gt = d.d_bytes + z.key_ok + z.tab_ok;
  a.pair_g1 = d.d_pair; a.pair_g2 = d.d_pair + m * 64;
  a.ws = d.d_ws; a.ws_status = d.d_ws_status;
  hipEvent_t evs[VKP_NUM_EVENTS];
  for (int i = 0; i < VKP_NUM_EVENTS; i++) evs[i] = d.ev[i];
  hipError_t e = bn254_launch_vkprep(a, s, stage_ms ? evs : nullptr);
  if (e != hipSuccess) { (void)hipStreamSynchronize(s); return launch_err(e, "verifying-key preparation"); }
  HIPCK(hipMemcpyAsync(d.h_out, d.d_out, z.dwords() * 4, hipMemcpyDeviceToHost, s));
  HIPCK(hipMemcpyAsync(d.h_bytes, d.d_bytes, z.bytes(), hipMemcpyDeviceToHost, s));
  HIPCK(hipStreamSynchronize(s));
  if (stage_ms)
    for (int i = 0; i + 1 < VKP_NUM_EVENTS; i++) { float ms = 0.f; if (hipEventElapsedTime(&ms, d.ev[i], d.ev[i + 1]) == hipSuccess) stage_ms[i] += ms; }
  p.g1pts = d.h_out; p.barg = d.h_out + z.g1pts; p.tabs = d.h_out + z.g1pts + z.barg;
  p.key_ok = d.h_bytes; p.tab_ok = d.h_bytes + z.key_ok; p.gt = d.h_bytes + z.key_ok + z.tab_ok;
  return BN254_OK;
}

// the host image of key j of a finished pass: field for field what prepare_g16 leaves (the K-point tables stay with the device that will use them)
void vkp_fill(G16Prepared& out, const VkpPass& p, size_t j) {
  const bn254::VkpKey k = p.keys[j];
  const size_t nk = k.g1_count - VKP_G1_FIXED;
  const int32_t* pts = p.g1pts + (size_t)k.g1_first * VKP_G1_DWORDS;
  out.n_k = nk;
  out.alpha.x = fp_from_limbs(pts); out.alpha.y = fp_from_limbs(pts + BN_NL);
  if (nk) { out.k0_pt.x = fp_from_limbs(pts + 3 * VKP_G1_DWORDS); out.k0_pt.y = fp_from_limbs(pts + 3 * VKP_G1_DWORDS + BN_NL); }
  else out.k0_pt = bn254::vkp_g1_generator();
  out.k0.resize(2 * BN_NL);
  fp_to_limbs(out.k0.data(), out.k0_pt.x); fp_to_limbs(out.k0.data() + BN_NL, out.k0_pt.y);
  out.b_arg = bn254::vkp_get_g2(p.barg + j * VKP_G2_DWORDS);
  const int32_t* tg = p.tabs + (2 * j) * (size_t)VKP_TAB_DWORDS;
  out.gtab.assign(tg, tg + VKP_TAB_DWORDS);
  out.dtab.assign(tg + VKP_TAB_DWORDS, tg + 2 * (size_t)VKP_TAB_DWORDS);
  out.target.resize(12 * BN_NL);
  const int korder[6] = {0, 2, 4, 1, 3, 5};
  const uint8_t* g = p.gt + 384 * j;
  for (int s = 0; s < 6; s++) {
    int32_t* o = out.target.data() + 2 * BN_NL * korder[s];
    fp_to_limbs(o, fp_from_be(g + 64 * s)); fp_to_limbs(o + BN_NL, fp_from_be(g + 64 * s + 32));
  }
  const size_t nb = out.key_inputs();
  out.msm_comb = g16_key_uses_comb(nb);
  if (nb) out.kpts.assign(pts + 4 * VKP_G1_DWORDS, pts + (4 + nb) * VKP_G1_DWORDS);
}

void vkp_free_all(bn254_g16_pvk** out, size_t n) { for (size_t i = 0; i < n; i++) { if (out[i]) bn254_groth16_vk_free(out[i]); out[i] = nullptr; } }

}  // namespace

// on_host: the lane bodies run on the host and no device is touched (the probe).  stage_ms (device passes; may be null): VKP_NUM_EVENTS - 1 sums over the passes, from
// HIP events
int vkp_prepare_batch(const uint8_t* const* vks, const size_t* vk_lens, size_t n_keys, unsigned mode, bool on_host, int device, bn254_g16_pvk** out, int* key_status,
                      float* stage_ms) {
  if (n_keys && (!vks || !vk_lens || !out || !key_status)) return set_err(BN254_E_BAD_ARG, "bad argument");
  if (mode > 1) return set_err(BN254_E_BAD_ARG, "bad argument: mode");
  for (size_t i = 0; i < n_keys; i++) if (!vks[i]) return set_err(BN254_E_BAD_ARG, "bad argument: null key in the list");
  for (size_t i = 0; i < n_keys; i++) { out[i] = nullptr; key_status[i] = BN254_E_VK; }
  if (stage_ms) for (int i = 0; i + 1 < VKP_NUM_EVENTS; i++) stage_ms[i] = 0.f;
  if (n_keys == 0) return BN254_OK;
  if (bn254_tables_on_host()) {
    // BN254_TABLES_HOST=1: the host construction of everything is what was asked for -- the single-key function, key by key
    for (size_t i = 0; i < n_keys; i++) {
      const int rc = bn254_groth16_vk_prepare(vks[i], vk_lens[i], mode, &out[i]);
      key_status[i] = rc;
      if (rc != BN254_OK && rc != BN254_E_VK) { const std::string keep = g_err; vkp_free_all(out, n_keys); return set_err(rc, keep); }
    }
    return BN254_OK;
  }
  if (!on_host) { int rc = check_device(device); if (rc || (rc = selftest_gate(device))) return rc; }
  try {
    VkpDev dev;
    VkpPass pass;
    size_t i = 0;
    while (i < n_keys || !pass.keys.empty()) {
      // the next pass: keys whose structure scans, until the pass is full; the others are BN254_E_VK already and get no lanes
      bool full = false;
      for (; i < n_keys && !full; i++) {
        G16VkLayout l;
        if (!scan_g16_vk(l, vks[i], vk_lens[i])) continue;
        const size_t need = VKP_G1_FIXED + (size_t)l.nk;
        if (!pass.keys.empty() && pass.n_g1 + need > VKP_PASS_G1) { full = true; break; }
        if (need > 0xffffffffu - pass.n_g1) { vkp_free_all(out, n_keys); return set_err(BN254_E_BAD_ARG, "a key with more than 2^32 points"); }
        vkp_add_key(pass, i, vks[i], l);
        if (pass.keys.size() >= g_vkp_pass_keys) { i++; full = true; break; }
      }
      if (pass.keys.empty()) break;
      int rc = BN254_OK;
      if (on_host) vkp_run_host(pass, (int)mode); else rc = vkp_run_device(pass, (int)mode, dev, stage_ms);
      if (rc) { const std::string keep = g_err; vkp_free_all(out, n_keys); return set_err(rc, keep); }
      for (size_t j = 0; j < pass.keys.size(); j++) {
        if (!(pass.key_ok[j] && pass.tab_ok[2 * j] && pass.tab_ok[2 * j + 1])) continue;
        bn254_g16_pvk* h = new (std::nothrow) bn254_g16_pvk();
        if (!h) { vkp_free_all(out, n_keys); return set_err(BN254_E_NOMEM, "out of memory"); }
        out[pass.key_of[j]] = h;
        vkp_fill(h->host, pass, j);
        key_status[pass.key_of[j]] = BN254_OK;
      }
      pass.clear();
    }
  } catch (const std::bad_alloc&) {
    vkp_free_all(out, n_keys);
    return set_err(BN254_E_NOMEM, "out of memory");
  }
  return BN254_OK;
}

extern "C" {

int bn254_groth16_vk_prepare_batch(const uint8_t* const* vks, const size_t* vk_lens, size_t n_keys, unsigned mode, int device, bn254_g16_pvk** out, int* key_status) {
  return vkp_prepare_batch(vks, vk_lens, n_keys, mode, false, device, out, key_status, nullptr);
}

}  // extern "C"
