"""The throughput form of the exact Groth16 path has no k_f12_conj, k_vm_init, k_g16_subgroup or k_g16_compare launches: conjugations ride on the load of the product
or squaring that consumes them (VE_CONJ, bn254_vm.h), the run kernel that starts the Miller loop sets f = 1 and T = (B, 1), the one that ends it tests B's subgroup
and resolves the deferred statuses, and the last product of the final exponentiation compares with the key's target.

CPU half (host simulator with the bound tracker, tests/hostsim/hostsim_fused.cpp): the program without conjugation operations against
bn254_pairing.h::final_exponentiation and, digit for digit, against the sequence it replaced; the folded init / subgroup test / comparison against the separate
operations.  GPU half: statuses of batches whose sub-batches take the Miller loop in 88, 44, 22 and 11 steps per launch, of a batch over several keys and of a
compressed batch, against the generator's expected bytes and the CPU oracle."""
import ctypes as C
import os
import random
import subprocess

import pytest

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 9                      # csrc/bn254_fp.h: BN_NL digits per field element


def be(v):
    return int(v).to_bytes(32, "big")


@pytest.fixture(scope="module")
def fused():
    """tests/hostsim/hostsim_fused.cpp: hostsim.cpp (bound tracker on) + the entry points of this file, compiled like tests/hostsim/Makefile compiles libhostsim.so"""
    d = os.path.join(ROOT, "tests", "hostsim")
    out = os.path.join(d, "libhostsim_fused.so")
    srcs = [os.path.join(d, f) for f in ("hostsim_fused.cpp", "hostsim.cpp", "hostsim_curve.inc")]
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O0", "-g", "-rdynamic", "-fno-inline", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                               "-Wno-unused-variable", "-shared", "-o", out, os.path.join(d, "hostsim_fused.cpp")])
    return C.CDLL(out)


def _vm_final_exp(hs, which, f, inflate=0):
    o = (C.c_uint8 * 384)(); digits = (C.c_int32 * (12 * NL))()
    hs.hs_vm_final_exp(which, o, digits, f, inflate)
    return bytes(o), list(digits)


def test_final_exp_program_without_conjugations(fused, O):
    """vm_final_exp_program == bn254_pairing.h::final_exponentiation (and the oracle's) on random values, lazily reduced inputs, Miller-loop outputs and edge values;
    VE_S0 holds the digits the sequence with explicit conjugations left there."""
    hs = fused
    rng = random.Random(0xF07D)
    r12 = lambda: b"".join(be(rng.randrange(P)) for _ in range(12))
    one = be(1) + bytes(352)
    g1, g2 = O.g1_gen(), O.g2_gen()
    cases = [(r12(), inf) for inf in (0, 1, 2) for _ in range(3)]
    cases += [(one, 0), (be(P - 1) + bytes(352), 0), (be(rng.randrange(1, P)) + bytes(352), 0)]                        # 1, -1, an element of Fp
    cases += [(r12()[:192] + bytes(192), 0), (bytes(192) + r12()[:192], 0)]                                             # c1 = 0 (conj(f) = f), c0 = 0 (conj(f) = -f)
    cases += [(be(rng.randrange(P)) + be(rng.randrange(P)) + bytes(320), 1), (bytes(64) + be(3) + bytes(288), 0)]      # an element of Fp2; v * 3
    for _ in range(2):
        pa, qb = O.g1_mul(g1, rng.randrange(1, R)), O.g2_mul(g2, rng.randrange(1, R))
        m = (C.c_uint8 * 384)()
        assert hs.hs_miller(m, pa, qb, 0, None, None) == 1
        cases.append((bytes(m), 0))
        cases.append((O.pairing(pa, qb), 0))                                                                             # already in the cyclotomic subgroup
    for f, inf in cases:
        want = (C.c_uint8 * 384)()
        hs.hs_final_exp(want, f)
        got, digits = _vm_final_exp(hs, 0, f, inf)
        assert got == bytes(want), (f.hex(), inf)
        assert got == O.final_exp(f), (f.hex(), inf)
        old, old_digits = _vm_final_exp(hs, 1, f, inf)
        assert old == got and old_digits == digits, (f.hex(), inf)


def _twist_point(O, rng):
    bt = O.fp2_op(2, O.fp2_op(3, (9, 1)), (3, 0))
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        rhs = O.fp2_op(0, O.fp2_op(2, O.fp2_op(5, x), x), bt)
        y = O.fp2_op(4, rhs)
        if y != (0, 0) and O.fp2_op(5, y) == rhs:
            return be(x[1]) + be(x[0]) + be(y[1]) + be(y[0])


def test_folded_init_subgroup_compare_equal_the_separate_operations(fused, O):
    """A pairing check with f = 1 / T = (B, 1), the r-torsion test of B and the comparison folded into the first run, the last run and the last product gives the
    verdicts and the GT element of the separate operations: every run length of the launch plans (88, 44, 22, 11) and one that does not divide the loop, accept,
    wrong pairing, B outside G2 (with the right and a wrong target), L at infinity."""
    hs = fused
    rng = random.Random(0xF01D)
    g1, g2 = O.g1_gen(), O.g2_gen()
    pa, pl, pc = (O.g1_mul(g1, rng.randrange(1, R)) for _ in range(3))
    qb, qg, qd = (O.g2_mul(g2, rng.randrange(1, R)) for _ in range(3))
    right = O.pairing(pa + pl + pc, qb + qg + qd)
    right_inf = O.pairing(pa + pc, qb + qd)
    wrong = O.pairing(pa + pl, qb + qg)
    off = _twist_point(O, rng)
    assert O.g2_subgroup_check(off) == 0

    def run(folded, per_run, B, l_inf, target):
        o = (C.c_uint8 * 384)()
        r = hs.hs_vm_g16_verdict(folded, per_run, pa, B, pl, qg, pc, qd, l_inf, target, o)
        assert r >= 0
        return r, bytes(o)

    for per_run in (0, 44, 22, 11, 7):
        for B, l_inf, target, want in ((qb, 0, right, 3), (qb, 0, wrong, 1), (qb, 1, right_inf, 3), (qb, 1, right, 1)):
            sep, folded = run(0, per_run, B, l_inf, target), run(1, per_run, B, l_inf, target)
            assert sep == folded and sep[0] == want, (per_run, l_inf, sep[0], folded[0])
            assert sep[1] == (right_inf if l_inf else right)
    for per_run in (0, 11):
        sep, folded = run(0, per_run, off, 0, right), run(1, per_run, off, 0, right)
        assert sep == folded and (sep[0] & 1) == 0, (per_run, sep[0], folded[0])
        # whatever the loop made of a point outside G2, a target equal to that value still compares equal in both forms: the verdict bit is the comparison alone
        sep2, folded2 = run(0, per_run, off, 0, sep[1]), run(1, per_run, off, 0, sep[1])
        assert sep2 == folded2 and sep2[0] == 2


# ---- GPU half ------------------------------------------------------------------------------------------------------------------------------------------------

def _oracle_sample(pkg, O, vk, proofs, inputs, n_public, st, n, per_class=6, stride_samples=24):
    """indices covering every status value present (per_class each) and an even stride over the batch; each against the oracle"""
    pick, seen = [], {}
    for i in range(n):
        c = seen.get(st[i], 0)
        if c < per_class:
            seen[st[i]] = c + 1; pick.append(i)
    pick += list(range(0, n, max(1, n // stride_samples))) + [n - 1]
    row = 32 * n_public
    for i in sorted(set(pick)):
        want = O.groth16_verify_many(proofs[256 * i:256 * i + 256], 256, vk, inputs[row * i:row * i + row], n_public, 1, O.MODE_REFERENCE)[0]
        assert st[i] == want, (i, st[i], want)


# 40 000: one sub-batch, the whole loop in one launch.  Above 65 536 proofs a batch runs as sub-batches side by side (bn254_g16_plan.h): with two of them 2^16 + 16 and
# 2^17 take 11 steps per launch, 200 000 takes 22 and 2^18 + 777 takes 44, so the first and the last launch of the loop are the same launch, neighbours, or far apart.
@pytest.mark.gpu
@pytest.mark.parametrize("n", [40000, (1 << 16) + 16, 1 << 17, 200000, (1 << 18) + 777])
def test_statuses_over_the_run_launch_plans(pkg, O, n):
    n_public = 2
    vk, proofs, inputs, exp = pkg.synth_groth16(0xF05E0000 + n, n_public, n, invalid_every=16, agree=True, threads=16)
    # every failure class: a point off the curve, a coordinate out of range, B outside G2, a wrong pairing
    assert set(exp) >= {pkg.ACCEPT, pkg.REJECT, pkg.ERR_NOT_IN_SUBGROUP, pkg.ERR_NOT_ON_CURVE, pkg.ERR_NOT_MEMBER}
    pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
    try:
        st = pvk.verify_batch(proofs, inputs, n, n_public=n_public)
        bad = [i for i in range(n) if st[i] != exp[i]]
        assert st == exp, (len(bad), [(i, st[i], exp[i]) for i in bad[:10]])
        _oracle_sample(pkg, O, vk, proofs, inputs, n_public, st, n)
        # a wrong input count is decided after the subgroup test (B outside G2 wins, then a deferred error of C, then INPUT_LEN): the statuses of the same records
        # with one input too few
        m = 5000
        short = pvk.verify_batch(proofs[:256 * m], bytes(32 * m), m, n_public=1)
        for i in range(m):
            want = exp[i] if exp[i] in (pkg.ERR_NOT_IN_SUBGROUP, pkg.ERR_NOT_ON_CURVE, pkg.ERR_NOT_MEMBER) else pkg.ERR_INPUT_LEN
            assert short[i] == want, (i, short[i], exp[i])
        for i in list(range(0, m, m // 10)) + [next(j for j in range(m) if exp[j] == c) for c in set(exp[:m])]:
            assert short[i] == O.groth16_verify_many(proofs[256 * i:256 * i + 256], 256, vk, bytes(32), 1, 1, O.MODE_REFERENCE)[0], i
        # strict scalars: an input >= r is NOT_MEMBER under the flag and the same input mod r without it
        rows = bytearray(inputs[:64 * m])
        hit = []
        for i in range(0, m, 7):
            x = int.from_bytes(rows[64 * i:64 * i + 32], "big")
            if x + R < 1 << 256:
                rows[64 * i:64 * i + 32] = (x + R).to_bytes(32, "big"); hit.append(i)
        assert len(hit) > m // 10
        strict = pvk.verify_batch(proofs[:256 * m], bytes(rows), m, n_public=n_public, flags=pkg.FLAG_STRICT_SCALARS)
        lax = pvk.verify_batch(proofs[:256 * m], bytes(rows), m, n_public=n_public)
        assert lax == exp[:m]
        hits = set(hit)
        for i in range(m):
            if i in hits and exp[i] in (pkg.ACCEPT, pkg.REJECT):
                assert strict[i] == pkg.ERR_NOT_MEMBER, i
            elif i not in hits:
                assert strict[i] == exp[i], i
    finally:
        pvk.close()


@pytest.mark.gpu
def test_statuses_of_a_batch_over_several_keys(pkg, O):
    """three keys with 0, 2 and 5 inputs, 90 000 proofs: two sub-batches, so the run that sets f and T and the run that tests B's subgroup are different launches of
    k_miller_run_keys, and the last product scatters the verdicts back to proof order"""
    from test_gpu_multikey import Key, Mixed
    keys = [Key(pkg, 0xF05E1000 + i, p, c, invalid_every=16) for i, (p, c) in enumerate(((0, 20000), (2, 45000), (5, 25000)))]
    try:
        mx = Mixed(keys, seed=5)
        st = mx.run(mx.key_set(pkg))
        bad = [i for i in range(len(st)) if st[i] != mx.exp[i]]
        assert st == mx.exp, (len(bad), [(i, mx.entries[i], st[i], mx.exp[i]) for i in bad[:10]])
        assert set(st) >= {pkg.ACCEPT, pkg.REJECT, pkg.ERR_NOT_IN_SUBGROUP, pkg.ERR_NOT_ON_CURVE, pkg.ERR_NOT_MEMBER}
        assert st == mx.per_key_calls()
        seen = {}
        for i, (k, _j) in enumerate(mx.entries):
            if seen.get((k, st[i]), 0) < 3:
                seen[(k, st[i])] = seen.get((k, st[i]), 0) + 1
                assert st[i] == mx.oracle(O, i), (i, mx.entries[i])
        assert len(seen) >= 12
    finally:
        for k in keys:
            k.pvk.close()


@pytest.mark.gpu
def test_statuses_of_a_compressed_batch(pkg, O):
    """BN254_FLAG_COMPRESSED_PROOFS over 70 000 records (two sub-batches): MALFORMED where a record does not decompress -- decided before the pipeline and kept --
    and the raw pipeline's byte elsewhere, which is the generator's expected byte for every record that was compressed from the generator's points"""
    from test_gpu_compressed import _compress_batch
    n_public, n = 2, 70000
    vk, proofs, inputs, exp = pkg.synth_groth16(0xF05E2000, n_public, n, invalid_every=16, agree=True, threads=16)
    pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
    try:
        recs, raw, pre = _compress_batch(pkg, proofs, n, 9, bad_every=11, invalid_every=16)
        st = pvk.verify_batch(recs, inputs, n, n_public=n_public, compressed=True)
        assert pre.count(1) > n // 20
        same = 0
        for i in range(n):
            if pre[i]:
                assert st[i] == pkg.ERR_MALFORMED, i
            elif raw[256 * i:256 * i + 256] == proofs[256 * i:256 * i + 256]:
                assert st[i] == exp[i], (i, st[i], exp[i]); same += 1
        assert same > n // 2 and set(st) >= {pkg.ACCEPT, pkg.REJECT, pkg.ERR_MALFORMED, pkg.ERR_NOT_IN_SUBGROUP}
        # the oracle reads raw records: every status present among the records that decompress, and a stride
        ok = [i for i in range(n) if not pre[i]]
        pick, seen = ok[::len(ok) // 24], {}
        for i in ok:
            if seen.get(st[i], 0) < 4:
                seen[st[i]] = seen.get(st[i], 0) + 1; pick.append(i)
        for i in sorted(set(pick)):
            assert st[i] == O.groth16_verify_many(raw[256 * i:256 * i + 256], 256, vk, inputs[64 * i:64 * i + 64], n_public, 1, O.MODE_REFERENCE)[0], i
    finally:
        pvk.close()
