// tests/hostsim/hostsim_expu.cpp -- TEST HARNESS: hostsim.cpp (the product's device arithmetic compiled for the host with the bound
// tracker on) plus the entry points tests/test_exp_u_chain.py needs for the exponentiation by u (bn254_vm.h::vm_exp_u):
//   - the operation sequence of vm_exp_u and of vm_final_exp_program as a TRACE (a recording OPS: no field arithmetic), which the test
//     replays on exponents in Python integers;
//   - vm_exp_u and vm_final_exp_program on values (HostOps: every operation asserts its digit and value bounds).
// Built by the test into libhostsim_expu.so; not part of the product.
#define HS_WITH_CURVE 1
#include "hostsim.cpp"

namespace {
const int KORDER[6] = {0, 2, 4, 1, 3, 5};   // tower byte order c0 = (k0, k2, k4), c1 = (k1, k3, k5) -> k index
void f12_to_ws(HostWs& w, int e, const uint8_t* b, int inflate) {
  for (int t = 0; t < 6; t++) { w.el[e + 2 * KORDER[t]] = fp_in(b + 64 * t, inflate); w.el[e + 2 * KORDER[t] + 1] = fp_in(b + 64 * t + 32, -inflate); }
}
void ws_to_f12(uint8_t* o, HostWs& w, int e) {
  for (int t = 0; t < 6; t++) { fp_out(o + 64 * t, w.el[e + 2 * KORDER[t]]); fp_out(o + 64 * t + 32, w.el[e + 2 * KORDER[t] + 1]); }
}
// one record per operation: {op, dst, a (with its VE_CONJ flag), b, arg}
enum { T_INV = 0, T_CONJ = 1, T_MUL = 2, T_FROB = 3, T_CYCLO_SQR = 4, T_CYCLO_SQR_N = 5 };
struct TraceOps {
  int32_t* out; int cap; int n;
  void rec(int op, int d, int a, int b, int arg) {
    if (n < cap) { int32_t* r = out + 5 * n; r[0] = op; r[1] = d; r[2] = a; r[3] = b; r[4] = arg; }
    n++;
  }
  void f12_inv(int d, int a) { rec(T_INV, d, a, -1, 0); }
  void f12_conj(int d, int a) { rec(T_CONJ, d, a, -1, 0); }
  void f12_mul(int d, int a, int b, bool conj_b = false) { rec(T_MUL, d, a, b, conj_b ? 1 : 0); }
  void f12_frob(int d, int a, int j) { rec(T_FROB, d, a, -1, j); }
  void f12_cyclo_sqr(int d, int a) { rec(T_CYCLO_SQR, d, a, -1, 1); }
  void f12_cyclo_sqr_n(int d, int a, int count) { rec(T_CYCLO_SQR_N, d, a, -1, count); }
};
}  // namespace

extern "C" {
// the workspace map the test needs: VE_F, VE_S0 .. VE_S4, the three table slots, VE_COUNT, VE_CONJ
void hs_expu_map(int32_t* o) {
  const int32_t m[11] = {VE_F, VE_S0, VE_S1, VE_S2, VE_S3, VE_S4, VE_UT0, VE_UT1, VE_UT2, VE_COUNT, VE_CONJ};
  for (int i = 0; i < 11; i++) o[i] = m[i];
}
// which 0: vm_exp_u(e_dst, e_src), 1: vm_final_exp_program.  Returns the number of operations (records of 5 ints; more than cap: the trace is cut).
int hs_expu_trace(int which, int e_dst, int e_src, int32_t* out, int cap) {
  TraceOps ops{out, cap, 0};
  if (which == 0) vm_exp_u(ops, e_dst, e_src); else vm_final_exp_program(ops);
  return ops.n;
}
// dst <- x^u on values: x (tower bytes) in e_src, the result of vm_exp_u from e_dst; every other element of the workspace starts as `fill` and is
// returned in `touched` (VE_COUNT flags: the element no longer holds `fill`)
void hs_expu_value(uint8_t* o, const uint8_t* x, int e_dst, int e_src, int inflate, uint8_t* touched) {
  static HostWs w;
  const Fp fill = fp_in(x + 32, 0);
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fill;
  f12_to_ws(w, e_src, x, inflate);
  HostWs before = w;
  HostOps ops{w, {nullptr, nullptr}, false};
  vm_exp_u(ops, e_dst, e_src);
  ws_to_f12(o, w, e_dst);
  for (int e = 0; e < VE_COUNT; e++) {
    bool same = true;
    for (int l = 0; l < BN_NL; l++) same = same && w.el[e].v[l] == before.el[e].v[l];
    touched[e] = same ? 0 : 1;
  }
}
// vm_final_exp_program on a value: VE_F <- f, the result from VE_S0
void hs_expu_final_exp(uint8_t* o, const uint8_t* f, int inflate) {
  static HostWs w;
  for (int e = 0; e < VE_COUNT; e++) w.el[e] = fp_zero();
  f12_to_ws(w, VE_F, f, inflate);
  HostOps ops{w, {nullptr, nullptr}, false};
  vm_final_exp_program(ops);
  ws_to_f12(o, w, VE_S0);
}
}
