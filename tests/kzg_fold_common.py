"""Vectors of the KZG batch-opening entry (include/bn254_verify.h: bn254_kzg_verify_folded_batch) for tests/test_kzg_fold_cpu.py and tests/test_gpu_kzg_fold.py.
The key is kzg_common's (g1 = s G1, g2 = b G2, tau_g2 = tau b G2 with s, b, tau known here).  A record opens k polynomials p_i at one point z with one quotient:
D_i = p_i(tau) g1, y_i = p_i(z), gamma restated from the reference's transcript.rs:68-107 / plonk/kzg.rs:46-72 with hashlib, H = (sum gamma^i (p_i(tau) - y_i)) /
(tau - z) g1.  Every point is a known multiple of the generator, so gamma, y^ = sum gamma^i y_i, the folded point and the expected status follow from Python integers,
hashlib.sha256 and the oracle's g1_mul alone; oracle_agrees() lets the oracle's pairing decide validity.  Built once per k and shared; nothing here calls the library.

A record with k = 1 does not depend on gamma (gamma^0 = 1), so the classes that reject THROUGH gamma -- swapped digests, a flipped data byte, the y_0 + d / y_1 - d
forgery -- exist for k >= 2 only; for k = 1 a flipped data byte is a valid record (class "data_flip_still_valid")."""
import hashlib
import random

import kzg_common as Z
import pairing_batch_common as V

R, P = V.R, V.P
KS = (1, 2, 3, 8, 13)
MAX_DIGESTS, MAX_DATA = 13, 64
MAIN_DATA_LEN = 5          # the data length of the main family of every k: odd, so a packed record is no multiple of 4 bytes
_CACHE = {}
_G1 = {}


def rec_len(k, data_len):
    return 96 + 96 * k + data_len


def g1_of(O, a):
    a %= R
    if a not in _G1:
        _G1[a] = Z.g1_of(O, a)
    return _G1[a]


def gamma_of(rec, k, data_len):
    """(digest, gamma) of a record's bytes as they stand: SHA-256("gamma" | be32(z mod r) | D_0 .. D_{k-1} | be32(y_i mod r) .. | data), big-endian, mod r"""
    z = int.from_bytes(rec[64 * k + 64:64 * k + 96], "big")
    ys = [int.from_bytes(rec[64 * k + 96 + 32 * i:64 * k + 128 + 32 * i], "big") for i in range(k)]
    data = rec[96 + 96 * k:96 + 96 * k + data_len]
    msg = b"gamma" + V.be(z % R) + rec[:64 * k] + b"".join(V.be(y % R) for y in ys) + data
    assert len(msg) == 37 + 96 * k + data_len
    d = hashlib.sha256(msg).digest()
    return d, int.from_bytes(d, "big") % R


class FVec:
    """One record: its bytes, k, data_len, the scalars ds, h (D_i = ds[i] G1, H = h G1 -- as they ARE in the record where its points are points), z and ys as encoded
    (possibly >= r), the decided loader error without / with FLAG_STRICT_SCALARS (None: the record reaches the pairing)"""

    def __init__(self, name, rec, k, data_len, ds, h, z, ys, err=None, strict_err=None):
        assert len(rec) == rec_len(k, data_len) and len(ds) == k and len(ys) == k
        self.name, self.rec, self.k, self.data_len, self.ds, self.h, self.z, self.ys, self.err, self.strict_err = name, rec, k, data_len, ds, h, z, ys, err, strict_err
        self.digest, self.gamma = gamma_of(rec, k, data_len)
        g = self.gamma
        self.yhat = sum(pow(g, i, R) * y for i, y in enumerate(ys)) % R
        # the opening this record folds to, in kzg_common's terms: its excess, points, weighted points and group sums are kzg_common's
        self.folded = Z.Vec(name, b"", sum(pow(g, i, R) * d for i, d in enumerate(ds)) % R, h % R, z, self.yhat, err, strict_err)


def status(K, v, strict=False):
    return Z.exact_status(K, v.folded, strict)


def enc(O, ds, h, z, ys, data):
    return b"".join(g1_of(O, d) for d in ds) + g1_of(O, h) + V.be(z) + b"".join(V.be(y) for y in ys) + bytes(data)


def proof(O, K, rng, k, data, z=None, coeffs=None, degree=3):
    """a valid record: (ds, h, z, ys) with the quotient for the gamma of these very bytes"""
    tau, s = K["tau"], K["s"]
    coeffs = [[rng.randrange(R) for _ in range(degree + 1)] for _ in range(k)] if coeffs is None else coeffs
    z = rng.randrange(R) if z is None else z
    at = lambda c, x: sum(a * pow(x, e, R) for e, a in enumerate(c)) % R
    ys, pt = [at(c, z) for c in coeffs], [at(c, tau) for c in coeffs]
    ds = [p * s % R for p in pt]
    _, g = gamma_of(enc(O, ds, 0, z, ys, data), k, len(data))      # H is not part of the transcript
    num = sum(pow(g, i, R) * (pt[i] - ys[i]) for i in range(k)) % R
    w = 0 if (tau - z) % R == 0 else num * pow((tau - z) % R, -1, R) % R
    assert (tau - z) % R or num == 0
    return ds, w * s % R, z, ys


def vectors(O, k):
    """(setup, main, extras): main -- the vectors of the main family (data_len MAIN_DATA_LEN, any mix of them is one call); extras -- [(data_len, [FVec])] with the data
    lengths that put the hashed length (37 + 96 k + data_len) at 55, 56, 63 and 0 mod 64, and 0 and 64.  At most 64 vectors in all"""
    if k in _CACHE:
        return _CACHE[k]
    K = Z.setup(O)
    rng = random.Random(0x4B5A4600 + k)
    main = []
    DL = MAIN_DATA_LEN

    def emit(name, ds, h, z, ys, data, rec=None, err=None, strict_err=None, into=main):
        v = FVec(name, enc(O, ds, h, z, ys, data) if rec is None else rec, k, len(data), [d % R for d in ds], h % R, z, ys, err, strict_err)
        into.append(v)
        return v

    def rdata(n=DL):
        return bytes(rng.randrange(256) for _ in range(n))

    for t in range(2):
        assert status(K, emit("valid%d" % t, *proof(O, K, rng, k, d := rdata()), d)) == V.ACCEPT
    ds, h, z, ys = proof(O, K, rng, k, d := rdata())
    for name, idx in (("value0_plus_one", 0), ("value_last_plus_one", k - 1)):
        if idx == 0 or k > 1:
            bad = list(ys); bad[idx] = (bad[idx] + 1) % R
            assert status(K, emit(name, ds, h, z, bad, d)) == V.REJECT
    good = enc(O, ds, h, z, ys, d)
    flipped = good[:-2] + bytes([good[-2] ^ 0x10]) + good[-1:]
    if k > 1:
        assert status(K, emit("digests_swapped", [ds[1], ds[0]] + ds[2:], h, z, ys, d)) == V.REJECT
        assert status(K, emit("data_byte_flipped", ds, h, z, ys, flipped[-DL:], rec=flipped)) == V.REJECT
        dd = rng.randrange(1, R)
        bad = [(ys[0] + dd) % R, (ys[1] - dd) % R] + ys[2:]
        assert sum(bad) % R == sum(ys) % R and status(K, emit("forgery_if_gamma_were_one", ds, h, z, bad, d)) == V.REJECT
    else:
        assert status(K, emit("data_flip_still_valid", ds, h, z, ys, flipped[-DL:], rec=flipped)) == V.ACCEPT
    # identity digests: the zero polynomial
    zero = [0, 0, 0, 0]
    rp = lambda: [rng.randrange(R) for _ in range(4)]
    for name, which in (("one_digest_identity", {k // 2}), ("all_digests_identity", set(range(k))), ("d0_identity", {0})):
        if name == "one_digest_identity" or k > 1:
            cs = [zero if i in which else rp() for i in range(k)]
            v = emit(name, *proof(O, K, rng, k, d := rdata(), coeffs=cs), d)
            assert status(K, v) == V.ACCEPT and all(v.ds[i] == 0 for i in which)
    # H the identity: constant polynomials
    ds, h, z, ys = proof(O, K, rng, k, d := rdata(), coeffs=[[rng.randrange(1, R)] for _ in range(k)])
    assert h == 0 and status(K, emit("h_identity", ds, h, z, ys, d)) == V.ACCEPT
    assert status(K, emit("h_identity_wrong", ds, h, z, [(ys[0] + 5) % R] + ys[1:], d)) == V.REJECT
    ds, h, z, ys = proof(O, K, rng, k, d := rdata(), coeffs=[[rng.randrange(1, R)] for _ in range(k)], z=K["tau"])
    assert h == 0 and status(K, emit("z_is_tau", ds, h, z, ys, d)) == V.ACCEPT
    assert status(K, emit("z_zero", *proof(O, K, rng, k, d := rdata(), z=0), d)) == V.ACCEPT
    # scalars >= r are used -- and hashed -- modulo r; strict: NOT_MEMBER
    ds, h, z, ys = proof(O, K, rng, k, d := rdata())
    v = emit("z_ge_r", ds, h, z + R, ys, d, strict_err=V.NOT_MEMBER)
    assert status(K, v) == V.ACCEPT and status(K, v, True) == V.NOT_MEMBER and v.z >= R
    v = emit("y_last_ge_r", ds, h, z, ys[:-1] + [ys[-1] + 4 * R], d, strict_err=V.NOT_MEMBER)
    assert status(K, v) == V.ACCEPT and v.ys[-1] < 2 ** 256
    v = emit("y0_ge_r_wrong", ds, h, z, [ys[0] + R + 1] + ys[1:], d, strict_err=V.NOT_MEMBER)
    assert status(K, v) == V.REJECT
    # range and curve checks in record order: D_0, D_{k-1}, H
    good = enc(O, ds, h, z, ys, d)

    def put(rec, off, field):
        return rec[:off] + field + rec[off + 32:]

    def bump(rec, off):
        return put(rec, off, V.be((int.from_bytes(rec[off:off + 32], "big") + 1) % P))

    oh, ol, oz = 64 * k, 64 * (k - 1), 64 * k + 64
    emit("d0_ge_p", ds, h, z, ys, d, rec=put(good, 0, V.be(P + 3)), err=V.NOT_MEMBER)
    emit("d0_off_curve", ds, h, z, ys, d, rec=bump(good, 32), err=V.NOT_ON_CURVE)
    if k > 1:
        emit("dlast_ge_p", ds, h, z, ys, d, rec=put(good, ol + 32, V.be(2 ** 256 - 1)), err=V.NOT_MEMBER)
        emit("dlast_off_curve", ds, h, z, ys, d, rec=bump(good, ol), err=V.NOT_ON_CURVE)
    emit("h_ge_p", ds, h, z, ys, d, rec=put(good, oh + 32, V.be(P)), err=V.NOT_MEMBER)
    emit("h_off_curve", ds, h, z, ys, d, rec=bump(good, oh), err=V.NOT_ON_CURVE)
    emit("order_digest_curve_before_h_ge_p", ds, h, z, ys, d, rec=put(bump(good, ol + 32), oh, V.be(P + 1)), err=V.NOT_ON_CURVE)
    emit("order_d0_ge_p_before_h_curve", ds, h, z, ys, d, rec=bump(put(good, 32, V.be(P + 1)), oh + 32), err=V.NOT_MEMBER)
    emit("order_range_first_inside_h", ds, h, z, ys, d, rec=put(bump(good, oh + 32), oh, V.be(P + 9)), err=V.NOT_MEMBER)
    emit("strict_beats_both", ds, h, z + R, ys, d, rec=put(put(bump(good, 32), oh, V.be(P)), oz, V.be(z + R)), err=V.NOT_ON_CURVE, strict_err=V.NOT_MEMBER)
    emit("strict_y_beats_ge_p", ds, h, z, ys[:-1] + [ys[-1] + R], d, rec=put(put(good, 0, V.be(P)), oz + 32 * k, V.be(ys[-1] + R)), err=V.NOT_MEMBER, strict_err=V.NOT_MEMBER)
    while len(main) < 36:
        ds, h, z, ys = proof(O, K, rng, k, d := rdata(), degree=rng.randrange(1, 4))
        if len(main) % 3 == 0:
            ys = ys[:-1] + [(ys[-1] + 7) % R]
        emit("fill%d" % len(main), ds, h, z, ys, d)
    # the data lengths that put the end of the message at the edges of SHA-256's padding: 55 (the last length with the padding in the same block), 56 (the first
    # that needs another), 63, 0 (a whole number of blocks) mod 64 -- at 37 + 96 k + data_len >= 133 these are the 119 / 120 / 127 / 128 cases of every later block
    extras, seen = [], {DL}
    for dl in [0, 64] + [(t - 37 - 96 * k) % 64 for t in (55, 56, 63, 0)]:
        if dl in seen:
            continue
        seen.add(dl)
        fam = []
        assert status(K, emit("valid_dl%d" % dl, *proof(O, K, rng, k, d := rdata(dl)), d, into=fam)) == V.ACCEPT
        ds, h, z, ys = proof(O, K, rng, k, d := rdata(dl))
        assert status(K, emit("wrong_dl%d" % dl, ds, h, z, [(ys[0] + 1) % R] + ys[1:], d, into=fam)) == V.REJECT
        extras.append((dl, fam))
    assert {(37 + 96 * k + dl) % 64 for dl in seen} >= {55, 56, 63, 0}
    assert len(main) + sum(len(f) for _, f in extras) <= 64 and len({v.name for v in main}) == len(main)
    _CACHE[k] = (K, main, extras)
    return _CACHE[k]


def batch(vecs, n, stride=None, start=0):
    """n records cycling through vecs (one family) from `start`: (buffer at `stride`, the FVec of each record)"""
    rl = len(vecs[0].rec)
    stride = rl if stride is None else stride
    idx = [(start + i) % len(vecs) for i in range(n)]
    return b"".join(vecs[j].rec + b"\xa5" * (stride - rl) for j in idx), [vecs[j] for j in idx]


def expected_fold(K, members, strict=False):
    """per record (digest, y^ as 32 bytes) as bn254_dbg_kzg_fold_proof reports them: zero bytes for a decided record"""
    return [(v.digest, V.be(v.yhat)) if status(K, v, strict) in (V.ACCEPT, V.REJECT) else (bytes(32), bytes(32)) for v in members]


def expected_points(O, K, members, strict=False, weights=None):
    return Z.expected_points(O, K, [v.folded for v in members], strict, weights)


def expected_rlc(O, K, members, weights, strict=False):
    return Z.expected_rlc(O, K, [v.folded for v in members], weights, strict)


def oracle_agrees(O, K, v):
    """the oracle's pairing on (F, g2), (-H, tau_g2), with F = sum gamma^i D_i - y^ g1 + z H built by the oracle's group operations from the record's OWN points (no
    identity among them), against the status the integers give: True when the oracle's product is 1 exactly where that status is ACCEPT"""
    k = v.k
    pts = [v.rec[64 * i:64 * i + 64] for i in range(k + 1)]
    assert all(any(p) for p in pts) and v.err is None
    F = O.g1_mul(K["g1"], (-v.yhat) % R)
    for i in range(k):
        F = O.g1_add(F, O.g1_mul(pts[i], pow(v.gamma, i, R)))
    F = O.g1_add(F, O.g1_mul(pts[k], v.z % R))
    nH = O.g1_mul(pts[k], R - 1)
    assert F == g1_of(O, Z.f_scalar(K, v.folded))
    gt = O.pairing(F + nH, K["g2"] + K["tau_g2"])
    return (gt == V.GT_ONE) == (status(K, v) == V.ACCEPT)


def forgery_pair(O, K, rng, k, data_len=MAIN_DATA_LEN):
    """two records whose quotients are off by amounts that cancel in an unweighted sum of the two checks (H is not part of the transcript, so gamma stays)"""
    a = proof(O, K, rng, k, da := bytes(rng.randrange(256) for _ in range(data_len)))
    b = proof(O, K, rng, k, db := bytes(rng.randrange(256) for _ in range(data_len)))
    tau = K["tau"]
    d = rng.randrange(1, R)
    db_h = d * ((a[2] - tau) % R) % R * pow((b[2] - tau) % R, -1, R) % R
    va = FVec("forged_a", enc(O, a[0], a[1] + d, a[2], a[3], da), k, data_len, a[0], (a[1] + d) % R, a[2], a[3])
    vb = FVec("forged_b", enc(O, b[0], b[1] - db_h, b[2], b[3], db), k, data_len, b[0], (b[1] - db_h) % R, b[2], b[3])
    ea, eb = Z.excess(K, va.folded), Z.excess(K, vb.folded)
    assert ea != 0 and eb != 0 and (ea + eb) % R == 0
    return va, vb
