"""Vectors of the pairing batch with shared, prepared G2 points (bn254_pairing_check_batch_shared) for tests/test_pairing_shared_cpu.py and
tests/test_gpu_pairing_shared.py: per shape (pair count, shared mask) the shared points Q_j = b_j G2, drawn once, and items that vary in G1 and in the variable Q, each
with the status the definition in include/bn254_verify.h gives the EXPANDED item and, where it reaches the pairing, the GT value -- both from the oracle and Python
integers, never from the product.  Built once per shape and shared; nothing here calls the library under test."""
import random

import pairing_batch_common as V

# (pairs, mask): one pair; the KZG shape; a shared point behind a variable one; one in front of two; the restated Groth16 shape; alternating kinds over all eight
# slots (with a shared IDENTITY at position 3); every slot shared
SHAPES = ((1, 0b1), (2, 0b11), (2, 0b10), (3, 0b001), (4, 0b1110), (8, 0b10101010), (8, 0xFF))
SHARED_IDENTITY = {(8, 0b10101010): 3}
CLASSES_ALWAYS = ("random", "identity", "identity_perturbed", "g1_identity_shared", "g1_ge_p_shared", "g1_off_curve_shared")
CLASSES_WITH_VARIABLE = ("g1_identity_variable", "g1_ge_p_variable", "g1_off_curve_variable", "order_", "g2_off_curve_variable", "g2_outside_subgroup_variable",
                         "subgroup_loses_to_curve")


def shared_positions(k, mask):
    return [j for j in range(k) if (mask >> j) & 1]


def variable_positions(k, mask):
    return [j for j in range(k) if not (mask >> j) & 1]


def packed_len(k, mask):
    return sum(64 if (mask >> j) & 1 else 192 for j in range(k))


_CACHE = {}


def vectors(O, k, mask):
    """(shared: {position: 128 bytes}, [(name, packed item, expanded item of 192 k bytes, expected status, expected GT bytes or None)])"""
    if (k, mask) in _CACHE:
        return _CACHE[(k, mask)]
    rng = random.Random(0x5A2ED + 256 * k + mask)
    g1, g2 = O.g1_gen(), O.g2_gen()
    sh, var = shared_positions(k, mask), variable_positions(k, mask)
    ident_at = SHARED_IDENTITY.get((k, mask))
    sb = {j: (0 if j == ident_at else rng.randrange(1, V.R)) for j in sh}              # the shared scalars b_j (0: the identity)
    shared = {j: (bytes(128) if sb[j] == 0 else O.g2_mul(g2, sb[j])) for j in sh}
    far = V.outside_g2(O, rng)
    out = []

    def g1_of(a):
        return bytes(64) if a % V.R == 0 else O.g1_mul(g1, a % V.R)

    def draw():
        """scalars and points of one item: a_j random, b_j the shared scalar or random"""
        a = [rng.randrange(1, V.R) for _ in range(k)]
        b = [sb[j] if j in sb else rng.randrange(1, V.R) for j in range(k)]
        return a, b, [g1_of(x) for x in a], [shared[j] if j in shared else O.g2_mul(g2, b[j]) for j in range(k)]

    def gt_of(ps, qs):
        keep = [j for j in range(k) if ps[j] != bytes(64) and qs[j] != bytes(128)]
        return O.pairing(b"".join(ps[j] for j in keep), b"".join(qs[j] for j in keep)) if keep else V.GT_ONE

    def emit(name, ps, qs, status=None, gt=False):
        for j in sh:
            assert qs[j] == shared[j], name             # a shared position never varies
        packed = b"".join(ps[j] + (b"" if j in shared else qs[j]) for j in range(k))
        expanded = b"".join(ps[j] + qs[j] for j in range(k))
        want = None
        if status is None:
            want = gt_of(ps, qs)
            status = V.ACCEPT if want == V.GT_ONE else V.REJECT
        assert len(packed) == packed_len(k, mask)
        out.append((name, packed, expanded, status, want))

    def put(b, j, off, field):
        """the 32-byte field at `off` of point j (G1 for off < 64, else the G2 half) replaced"""
        ps, qs = b
        ps, qs = list(ps), list(qs)
        if off < 64:
            ps[j] = ps[j][:off] + field + ps[j][off + 32:]
        else:
            o = off - 64
            qs[j] = qs[j][:o] + field + qs[j][o + 32:]
        return ps, qs

    def bump(b, j, off):
        """that field plus one mod p: off the curve (checked by the expectation itself)"""
        ps, qs = b
        src = ps[j] if off < 64 else qs[j]
        o = off if off < 64 else off - 64
        return put(b, j, off, V.be((int.from_bytes(src[o:o + 32], "big") + 1) % V.P))

    # random items: the oracle's GT value, not 1
    for t in range(2):
        _, _, ps, qs = draw()
        emit("random%d" % t, ps, qs)
        assert out[-1][3] == V.REJECT
    # a bilinear identity sum a_j b_j = 0 over the positions that contribute, solved for the last contributing position; then the same perturbed by one
    a, b, ps, qs = draw()
    last = max(j for j in range(k) if b[j] != 0)
    s = sum(a[j] * b[j] for j in range(k) if j != last) % V.R
    a[last] = (V.R - s) * pow(b[last], -1, V.R) % V.R
    ps[last] = g1_of(a[last])
    emit("identity", ps, qs)
    assert out[-1][3] == V.ACCEPT and out[-1][4] == V.GT_ONE
    ps[last] = g1_of(a[last] + 1)
    emit("identity_perturbed", ps, qs)
    assert out[-1][3] == V.REJECT
    # an identity of G1 at a shared and at a variable position: that pair contributes 1
    for kind, pos in (("shared", sh), ("variable", var)):
        if pos:
            _, _, ps, qs = draw()
            ps[pos[-1]] = bytes(64)
            emit("g1_identity_%s" % kind, ps, qs)
    # the range and curve checks of G1 at a shared and at a variable position
    for kind, pos in (("shared", sh), ("variable", var)):
        if pos:
            j = pos[0]
            _, _, ps, qs = draw()
            emit("g1_ge_p_%s" % kind, *put((ps, qs), j, 0, V.be(V.P + 5)), status=V.NOT_MEMBER)
            emit("g1_off_curve_%s" % kind, *bump((ps, qs), j, 32), status=V.NOT_ON_CURVE)
    if ident_at is not None:
        # the G1 point beside a shared identity is still validated
        _, _, ps, qs = draw()
        emit("g1_off_curve_beside_shared_identity", *bump((ps, qs), ident_at, 32), status=V.NOT_ON_CURVE)
    if var:
        v = var[0]
        _, _, ps, qs = draw()
        emit("g2_off_curve_variable", *bump((ps, qs), v, 64 + 96), status=V.NOT_ON_CURVE)
        emit("g2_ge_p_variable", *put((ps, qs), var[-1], 64 + 32, V.be(2 ** 256 - 1)), status=V.NOT_MEMBER)
        qs2 = list(qs); qs2[v] = far
        emit("g2_outside_subgroup_variable", ps, qs2, status=V.NOT_IN_SUBGROUP)
        # phase 2 loses to phase 1: a curve failure at a later position (any position, where the variable one is the last)
        later = [j for j in range(k) if j > v] or [j for j in range(k) if j != v]
        if later:
            emit("subgroup_loses_to_curve", *bump((ps, qs2), later[-1], 32), status=V.NOT_ON_CURVE)
        else:
            emit("subgroup_loses_to_curve", *bump((ps, qs2), v, 32), status=V.NOT_ON_CURVE)
        # record order across a shared and a variable position, whichever ways round the shape has: the first failure decides, the later one is of the other kind
        orders = [(s_, v_) for s_ in sh for v_ in var if s_ < v_][:1] + [(v_, s_) for v_ in var for s_ in sh if v_ < s_][:1]
        for first, second in orders:
            tag = "order_%s%d_before_%s%d" % ("s" if first in shared else "v", first, "s" if second in shared else "v", second)
            _, _, ps, qs = draw()

            def off_curve(b, j):
                return bump(b, j, 32) if j in shared else bump(b, j, 64 + 96)     # a shared position has only its G1 point to fail with

            def ge_p(b, j):
                return put(b, j, 32, V.be(V.P)) if j in shared else put(b, j, 64 + 64, V.be(V.P + 1))

            emit(tag + "_curve_first", *ge_p(off_curve((ps, qs), first), second), status=V.NOT_ON_CURVE)
            emit(tag + "_member_first", *off_curve(ge_p((ps, qs), first), second), status=V.NOT_MEMBER)
    assert len(out) <= 64
    _CACHE[(k, mask)] = (shared, out)
    return _CACHE[(k, mask)]


def classes_of(k, mask):
    """the classes a shape can produce (name prefixes)"""
    c = list(CLASSES_ALWAYS)
    if variable_positions(k, mask):
        c += list(CLASSES_WITH_VARIABLE)
    return c


def statuses_of(k, mask):
    s = {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE}
    if variable_positions(k, mask):
        s.add(V.NOT_IN_SUBGROUP)
    return s


def batch(vecs, n, k, mask, item_stride=None, start=0):
    """n items cycling through vecs from `start`: (packed buffer at item_stride, expanded buffer of 192 k bytes per item, expected status bytes, indices)"""
    rec = packed_len(k, mask)
    stride = rec if item_stride is None else item_stride
    idx = [(start + i) % len(vecs) for i in range(n)]
    packed = b"".join(vecs[j][1] + b"\xa5" * (stride - rec) for j in idx)
    expanded = b"".join(vecs[j][2] for j in idx)
    return packed, expanded, bytes(vecs[j][3] for j in idx), idx
