"""Vectors of the KZG batch (include/bn254_verify.h: bn254_kzg_key_prepare, bn254_kzg_verify_batch) for tests/test_kzg_cpu.py and tests/test_gpu_kzg.py.  The key is
g1 = s G1 (s != 1), g2 = b G2, tau_g2 = tau b G2 with s, b and tau known here; every point of an opening is a known multiple of the generator, so the expected status,
the expected F_i = C_i - y_i g1 + z_i H_i and the group sums follow from Python integers and the oracle's g1_mul alone -- never from the product.  Built once and
shared; nothing here calls the library under test."""
import random

import pairing_batch_common as V

R, P = V.R, V.P
PENDING = 0x80          # "reaches the pairing": only inside this file
_CACHE = {}


class Vec:
    """One opening: its bytes, the scalars c, h (C = c G1, H = h G1), z and y AS ENCODED (possibly >= r), the status without and with FLAG_STRICT_SCALARS; err is
    the decided loader error, or None when the opening reaches the pairing"""

    def __init__(self, name, rec, c, h, z, y, err, strict_err):
        self.name, self.rec, self.c, self.h, self.z, self.y, self.err, self.strict_err = name, rec, c, h, z, y, err, strict_err


def g1_of(O, a):
    a %= R
    return bytes(64) if a == 0 else O.g1_mul(O.g1_gen(), a)


def setup(O):
    """{"s", "b", "tau", "g1", "g2", "tau_g2"} of the vectors' key"""
    if "setup" not in _CACHE:
        rng = random.Random(0x4B5A47)
        s, b, tau = rng.randrange(2, R), rng.randrange(2, R), rng.randrange(2, R)
        _CACHE["setup"] = {"s": s, "b": b, "tau": tau, "g1": g1_of(O, s), "g2": O.g2_mul(O.g2_gen(), b), "tau_g2": O.g2_mul(O.g2_gen(), tau * b % R)}
    return _CACHE["setup"]


def excess(K, v):
    """e_i with e(F_i, g2) e(-H_i, tau_g2) = e(G1, g2)^(e_i): the opening verifies exactly when it is 0 mod r"""
    return (v.c - v.y * K["s"] + v.z * v.h - K["tau"] * v.h) % R


def f_scalar(K, v, weight=1):
    return weight * (v.c - v.y * K["s"] + v.z * v.h) % R


def exact_status(K, v, strict=False):
    if strict and v.strict_err is not None:
        return v.strict_err
    if v.err is not None:
        return v.err
    return V.ACCEPT if excess(K, v) == 0 else V.REJECT


def opening(O, K, rng, degree=3, z=None, coeffs=None):
    """a valid opening of a random polynomial p (coefficients in units of g1): (c, h, z, y) with C = p(tau) g1, H = ((p(tau) - y) / (tau - z)) g1, y = p(z)"""
    tau, s = K["tau"], K["s"]
    coeffs = [rng.randrange(R) for _ in range(degree + 1)] if coeffs is None else coeffs
    z = rng.randrange(R) if z is None else z
    at = lambda x: sum(a * pow(x, e, R) for e, a in enumerate(coeffs)) % R
    y, ptau = at(z), at(tau)
    w = 0 if (tau - z) % R == 0 else (ptau - y) * pow((tau - z) % R, -1, R) % R
    return ptau * s % R, w * s % R, z, y


def enc(O, c, h, z, y):
    return g1_of(O, c) + g1_of(O, h) + V.be(z) + V.be(y)


def vectors(O):
    """(setup, [Vec]): at most 64, every class of the issue"""
    if "vectors" in _CACHE:
        return _CACHE["vectors"]
    K = setup(O)
    rng = random.Random(0x4B5A4701)
    out = []

    def emit(name, c, h, z, y, rec=None, err=None, strict_err=None):
        v = Vec(name, enc(O, c, h, z, y) if rec is None else rec, c % R, h % R, z, y, err, strict_err)
        out.append(v)
        return v

    for t in range(3):
        assert exact_status(K, emit("valid%d" % t, *opening(O, K, rng))) == V.ACCEPT
    c, h, z, y = opening(O, K, rng)
    assert exact_status(K, emit("value_plus_one", c, h, z, (y + 1) % R)) == V.REJECT
    assert exact_status(K, emit("wrong_quotient", c, (h + K["s"]) % R, z, y)) == V.REJECT
    # scalars >= r are used modulo r; strict: NOT_MEMBER
    c, h, z, y = opening(O, K, rng)
    for name, zz, yy in (("z_ge_r", z + R, y), ("y_ge_r", z, y + 4 * R), ("both_ge_r", z + 4 * R, y + R)):
        assert zz < 2 ** 256 and yy < 2 ** 256
        v = emit(name, c, h, zz, yy, strict_err=V.NOT_MEMBER)
        assert exact_status(K, v) == V.ACCEPT and exact_status(K, v, True) == V.NOT_MEMBER
    v = emit("z_ge_r_wrong", c, h, z + R, y + R + 1, strict_err=V.NOT_MEMBER)
    assert exact_status(K, v) == V.REJECT
    # y = 0: p = (X - z) q
    z = rng.randrange(1, R)
    q = [rng.randrange(R) for _ in range(3)]
    coeffs = [(-z * q[0]) % R] + [(q[e - 1] - z * q[e]) % R for e in (1, 2)] + [q[2]]
    c, h, zz, y = opening(O, K, rng, coeffs=coeffs, z=z)
    assert y == 0 and exact_status(K, emit("y_zero", c, h, zz, y)) == V.ACCEPT
    assert exact_status(K, emit("z_zero", *opening(O, K, rng, z=0))) == V.ACCEPT
    # z = tau: the quotient's denominator vanishes -- the constant polynomial, H the identity (then F is the identity too)
    c, h, z, y = opening(O, K, rng, coeffs=[rng.randrange(1, R)], z=K["tau"])
    assert h == 0 and f_scalar(K, Vec("", b"", c, h, z, y, None, None)) == 0 and exact_status(K, emit("z_is_tau", c, h, z, y)) == V.ACCEPT
    assert exact_status(K, emit("c_identity", 0, 0, rng.randrange(R), 0)) == V.ACCEPT        # the zero polynomial
    c, h, z, y = opening(O, K, rng, coeffs=[rng.randrange(1, R)])
    assert h == 0 and exact_status(K, emit("h_identity", c, h, z, y)) == V.ACCEPT
    assert exact_status(K, emit("h_identity_wrong", c, h, z, (y + 5) % R)) == V.REJECT
    # F the identity while H is not: e(-H, tau_g2) alone, not 1
    h, z, y = rng.randrange(1, R), rng.randrange(R), rng.randrange(R)
    v = emit("f_identity", (y * K["s"] - z * h) % R, h, z, y)
    assert f_scalar(K, v) == 0 and exact_status(K, v) == V.REJECT
    # range and curve checks, record order
    c, h, z, y = opening(O, K, rng)
    good = enc(O, c, h, z, y)

    def put(rec, off, field):
        return rec[:off] + field + rec[off + 32:]

    def bump(rec, off):
        return put(rec, off, V.be((int.from_bytes(rec[off:off + 32], "big") + 1) % P))

    emit("c_ge_p", c, h, z, y, rec=put(good, 0, V.be(P + 3)), err=V.NOT_MEMBER)
    emit("h_ge_p", c, h, z, y, rec=put(good, 96, V.be(2 ** 256 - 1)), err=V.NOT_MEMBER)
    emit("c_off_curve", c, h, z, y, rec=bump(good, 32), err=V.NOT_ON_CURVE)
    emit("h_off_curve", c, h, z, y, rec=bump(good, 64), err=V.NOT_ON_CURVE)
    emit("order_c_curve_before_h_ge_p", c, h, z, y, rec=put(bump(good, 32), 64, V.be(P)), err=V.NOT_ON_CURVE)
    emit("order_c_ge_p_before_h_curve", c, h, z, y, rec=bump(put(good, 32, V.be(P + 1)), 96), err=V.NOT_MEMBER)
    emit("order_h_ge_p_after_good_c", c, h, z, y, rec=put(bump(good, 96), 64, V.be(P + 9)), err=V.NOT_MEMBER)      # inside one point the range check comes first
    # a strict scalar error together with a curve error: the strict error wins
    emit("strict_beats_curve", c, h, z + R, y, rec=put(bump(good, 32), 128, V.be(z + R)), err=V.NOT_ON_CURVE, strict_err=V.NOT_MEMBER)
    emit("strict_beats_ge_p", c, h, z, y + R, rec=put(put(good, 64, V.be(P)), 160, V.be(y + R)), err=V.NOT_MEMBER, strict_err=V.NOT_MEMBER)
    while len(out) < 30:
        c, h, z, y = opening(O, K, rng, degree=rng.randrange(1, 4))
        wrong = len(out) % 3 == 0
        emit("fill%d" % len(out), c, h, z, (y + (7 if wrong else 0)) % R)
    assert len(out) <= 64 and len({v.name for v in out}) == len(out)
    _CACHE["vectors"] = (K, out)
    return _CACHE["vectors"]


def status_classes(K, vecs, strict=False):
    return {exact_status(K, v, strict) for v in vecs}


def batch(vecs, n, stride=192, start=0):
    """n openings cycling through vecs from `start`: (buffer at `stride`, the Vec of each opening)"""
    idx = [(start + i) % len(vecs) for i in range(n)]
    return b"".join(vecs[j].rec + b"\xa5" * (stride - 192) for j in idx), [vecs[j] for j in idx]


def expected_points(O, K, members, strict=False, weights=None):
    """per opening (F bytes, H' bytes, (F identity, H' identity)) as bn254_dbg_kzg_fold reports them: zero bytes and no flag for a decided opening.  weights None: the
    exact form (F_i, -H_i); else F'_i = r_i F_i and H'_i = -r_i H_i"""
    memo = {}
    out = []
    for i, v in enumerate(members):
        if exact_status(K, v, strict) not in (V.ACCEPT, V.REJECT):
            out.append((bytes(64), bytes(64), (0, 0)))
            continue
        w = 1 if weights is None else weights[i] | 1
        fs, hs = f_scalar(K, v, w), (-w * v.h) % R
        for a in (fs, hs):
            if a not in memo:
                memo[a] = g1_of(O, a)
        out.append((memo[fs], memo[hs], (int(fs == 0), int(hs == 0))))
    return out


def expected_rlc(O, K, members, weights, strict=False):
    """(status bytes of the weighted path under these weights, [(F sum, H sum, flags, group status)] per 64 openings, failed groups): a group passes when the weighted
    excesses of its pending openings sum to 0 -- then ALL of them are accepted; the openings of a failed group get their own verdict"""
    st = [exact_status(K, v, strict) for v in members]
    groups, failed = [], 0
    for g in range(0, len(members), 64):
        pend = [i for i in range(g, min(g + 64, len(members))) if st[i] in (V.ACCEPT, V.REJECT)]
        fs = sum(f_scalar(K, members[i], weights[i] | 1) for i in pend) % R
        hs = sum(-(weights[i] | 1) * members[i].h for i in pend) % R
        ok = (fs + K["tau"] * hs) % R == 0
        if pend and not ok:
            failed += 1
        groups.append((g1_of(O, fs), g1_of(O, hs), (int(fs == 0), int(hs == 0)) if pend else (0, 0), V.ACCEPT if ok else V.REJECT))
        if ok:
            for i in pend:
                st[i] = V.ACCEPT
    return bytes(st), groups, failed


def forgery_pair(O, K, rng):
    """two openings that claim v_a + d and v_b - d: their errors cancel in an unweighted sum"""
    a, b = opening(O, K, rng), opening(O, K, rng)
    d = rng.randrange(1, R)
    va = Vec("forged_a", enc(O, a[0], a[1], a[2], (a[3] + d) % R), a[0], a[1], a[2], (a[3] + d) % R, None, None)
    vb = Vec("forged_b", enc(O, b[0], b[1], b[2], (b[3] - d) % R), b[0], b[1], b[2], (b[3] - d) % R, None, None)
    assert excess(K, va) != 0 and excess(K, vb) != 0 and (excess(K, va) + excess(K, vb)) % R == 0
    return va, vb
