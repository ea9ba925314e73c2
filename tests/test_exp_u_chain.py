"""The exponentiation by u of the final exponentiation (bn254_vm.h::vm_exp_u) runs an addition-subtraction chain described as data
(csrc/bn254_constants.h: BN_U_CHAIN_*, written by gen_constants.py, found by tools/search_u_chain.py): 61 cyclotomic squarings and 14 products
instead of the 63 and 16 of width-4 signed windows.

The operation sequence the GPU runs is recorded on the host (tests/hostsim/hostsim_expu.cpp: an OPS that writes a trace instead of doing field
arithmetic) and replayed here on EXPONENTS in Python integers: vm_exp_u must give exactly u within its operation budget and touch nothing but
its destination and the three table slots, and vm_final_exp_program must still raise to the exponent it raised to before.  The same harness
runs both on values under the bound tracker (the operand pairings of the products are new) against the oracle."""
import ctypes as C
import math
import os
import random
import subprocess
import sys

import pytest

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
U = 4965661367192848881
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHI12 = P**4 - P**2 + 1                   # order of the cyclotomic subgroup, where vm_exp_u works: conj(x) = x^(p^6) = x^-1 there
EASY = (P**6 - 1) * (P**2 + 1)
GROUP = P**12 - 1
MAX_PRODUCTS, MAX_SQUARINGS, LONGEST_RUN = 14, 61, 7
T_INV, T_CONJ, T_MUL, T_FROB, T_CYCLO_SQR, T_CYCLO_SQR_N = range(6)


def be(v):
    return int(v).to_bytes(32, "big")


@pytest.fixture(scope="module")
def expu():
    """tests/hostsim/hostsim_expu.cpp: hostsim.cpp (bound tracker on) + the entry points of this file, compiled like tests/hostsim/Makefile compiles libhostsim.so"""
    d = os.path.join(ROOT, "tests", "hostsim")
    out = os.path.join(d, "libhostsim_expu.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_expu.cpp", "hostsim.cpp", "hostsim_curve.inc")]
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O0", "-g", "-rdynamic", "-fno-inline", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                               "-Wno-unused-variable", "-shared", "-o", out, os.path.join(d, "hostsim_expu.cpp")])
    hs = C.CDLL(out)
    m = (C.c_int32 * 11)()
    hs.hs_expu_map(m)
    hs.ve = dict(zip(("F", "S0", "S1", "S2", "S3", "S4", "UT0", "UT1", "UT2", "COUNT", "CONJ"), list(m)))
    return hs


def _trace(hs, which, e_dst=0, e_src=0):
    cap = 400
    buf = (C.c_int32 * (5 * cap))()
    n = hs.hs_expu_trace(which, e_dst, e_src, buf, cap)
    assert 0 < n <= cap
    return [tuple(buf[5 * i:5 * i + 5]) for i in range(n)]


def _replay(trace, slots, conj, mod, inv=None):
    """The trace on exponents.  slots: {element: exponent}; conj: what a conjugation multiplies an exponent by; inv likewise for f12_inv.
    Reading a slot nothing wrote is an error (KeyError)."""
    CONJ = 0x100
    for op, d, a, b, arg in trace:
        x = slots[a & ~CONJ] * (conj if a & CONJ else 1)
        if op == T_INV:
            v = x * inv
        elif op == T_CONJ:
            v = x * conj
        elif op == T_MUL:
            v = x + slots[b] * (conj if arg else 1)
        elif op == T_FROB:
            v = x * P**arg
        else:
            v = x << arg
        slots[d] = v % mod if mod else v
    return slots


def test_chain_description_is_checked_where_it_is_generated():
    """gen_constants.py asserts the chain in Python integers (it evaluates to u, runs of at most 7, at most three table entries) and the committed header is its output"""
    sys.path.insert(0, os.path.join(ROOT, "snark-bn254-verifier_amd"))
    try:
        import gen_constants as G
    finally:
        sys.path.pop(0)
    c = G.u_chain()
    assert (c["squarings"], c["products"]) == (61, 14) and len(c["table"]) <= 3 and max(c["runs"]) <= LONGEST_RUN
    r = subprocess.run([sys.executable, os.path.join(ROOT, "snark-bn254-verifier_amd", "gen_constants.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc", "bn254_constants.h")).read()


def test_exp_u_raises_to_u_within_its_budget(expu):
    """every (destination, source) pair the final exponentiation uses, and one more"""
    ve = expu.ve
    assert ve["CONJ"] == 0x100
    table = {ve["UT0"], ve["UT1"], ve["UT2"]}
    for e_dst, e_src in ((ve["S0"], ve["F"]), (ve["S2"], ve["S1"]), (ve["S4"], ve["S3"]), (ve["F"], ve["S4"])):
        tr = _trace(expu, 0, e_dst, e_src)
        # exponents as plain integers, a conjugation is a negation: exactly u, not u modulo something
        slots = _replay(tr, {e_src: 1}, -1, None)
        assert slots[e_dst] == U
        products = sum(1 for t in tr if t[0] == T_MUL)
        squarings = sum(t[4] for t in tr if t[0] in (T_CYCLO_SQR, T_CYCLO_SQR_N))
        assert products <= MAX_PRODUCTS and squarings <= MAX_SQUARINGS, (products, squarings)
        assert all(t[0] in (T_MUL, T_CYCLO_SQR, T_CYCLO_SQR_N) for t in tr)
        assert all(1 <= t[4] <= LONGEST_RUN for t in tr if t[0] == T_CYCLO_SQR_N) and all(t[4] == 1 for t in tr if t[0] == T_CYCLO_SQR)
        # writes: the destination and the three table slots only, and never a flagged index; reads: those and the source
        assert {t[1] for t in tr} <= table | {e_dst}
        assert {t[2] & ~0x100 for t in tr} | {t[3] for t in tr if t[0] == T_MUL} <= table | {e_dst, e_src}
        # a general product may overwrite its first operand, never its second
        assert all(t[1] != t[3] for t in tr if t[0] == T_MUL)


def test_final_exp_program_keeps_its_exponent(expu):
    ve = expu.ve
    tr = _trace(expu, 1)
    slots = _replay(tr, {ve["F"]: 1}, P**6, GROUP, inv=-1)
    # the hard part as the program's comments state it (Fuentes-Castaneda et al.): lambda_0 + lambda_1 p + lambda_2 p^2 + lambda_3 p^3
    u = U
    hard = (12 * u**3 + 12 * u**2 + 6 * u + 1) + P * (12 * u**3 + 6 * u**2 + 4 * u) + P**2 * (12 * u**3 + 6 * u**2 + 6 * u) + P**3 * (12 * u**3 + 6 * u**2 + 4 * u - 1)
    assert slots[ve["S0"]] == EASY * (hard % PHI12) % GROUP
    # and that exponent is a multiple of (p^4 - p^2 + 1) / r by a factor prime to r: a final exponentiation
    assert PHI12 % R == 0 and hard % (PHI12 // R) == 0 and math.gcd(hard // (PHI12 // R), R) == 1
    # three exponentiations by u make up all but 12 products and 6 squarings of it
    assert sum(1 for t in tr if t[0] == T_MUL) <= 12 + 3 * MAX_PRODUCTS
    assert sum(t[4] for t in tr if t[0] in (T_CYCLO_SQR, T_CYCLO_SQR_N)) <= 3 + 3 * MAX_SQUARINGS
    written = {t[1] for t in tr}
    assert written <= {ve[k] for k in ("F", "S0", "S1", "S2", "S3", "S4", "UT0", "UT1", "UT2")}


def _cyclotomic(O, f):
    """f^((p^6 - 1)(p^2 + 1)) with the oracle's operations (test_hostsim.py: 7 conjugation, 2 inversion, 4 Frobenius p^2, 0 product)"""
    c = O.fp12_op(0, O.fp12_op(7, f), O.fp12_op(2, f))
    return O.fp12_op(0, O.fp12_op(4, c), c)


def _pow(O, x, e):
    r = None
    for bit in bin(e)[2:]:
        if r is not None:
            r = O.fp12_op(0, r, r)
        if bit == "1":
            r = x if r is None else O.fp12_op(0, r, x)
    return r


def test_values_under_the_bound_tracker(expu, O):
    """vm_exp_u on elements of the cyclotomic subgroup, canonical and lazily reduced, against square-and-multiply with the oracle's product; the whole
    program against the oracle's final_exponentiation on random Fp12 values and edge values.  Every operation asserts its bounds (BN_TRACK_BOUNDS)."""
    hs, ve = expu, expu.ve
    rng = random.Random(0xE0B5)
    r12 = lambda: b"".join(be(rng.randrange(P)) for _ in range(12))
    one = be(1) + bytes(352)
    table = {ve["UT0"], ve["UT1"], ve["UT2"]}
    for e_dst, e_src, inflate in ((ve["S0"], ve["F"], 0), (ve["S2"], ve["S1"], 1), (ve["S4"], ve["S3"], 2)):
        x = _cyclotomic(O, r12())
        o = (C.c_uint8 * 384)(); touched = (C.c_uint8 * ve["COUNT"])()
        hs.hs_expu_value(o, x, e_dst, e_src, inflate, touched)
        assert bytes(o) == _pow(O, x, U)
        allowed = {s + k for s in table | {e_dst} for k in range(12)}
        assert {e for e in range(ve["COUNT"]) if touched[e]} <= allowed
    o = (C.c_uint8 * 384)(); touched = (C.c_uint8 * ve["COUNT"])()
    hs.hs_expu_value(o, one, ve["S0"], ve["F"], 0, touched)
    assert bytes(o) == one
    cases = [(r12(), inf) for inf in (0, 1, 2) for _ in range(3)]
    cases += [(one, 0), (be(P - 1) + bytes(352), 0), (r12()[:192] + bytes(192), 0), (bytes(192) + r12()[:192], 0)]
    g1, g2 = O.g1_gen(), O.g2_gen()
    cases.append((O.miller_loop(O.g1_mul(g1, rng.randrange(1, R)), O.g2_mul(g2, rng.randrange(1, R))), 0))
    for f, inf in cases:
        hs.hs_expu_final_exp(o, f, inf)
        assert bytes(o) == O.final_exp(f), (f.hex(), inf)
