"""Vectors of the batch pairing product (bn254_pairing_check_batch) for tests/test_pairing_batch_cpu.py and tests/test_gpu_pairing_batch.py: items of k pairs with
the status the definition in include/bn254_verify.h gives them and, where an item reaches the pairing, the GT value -- both from the oracle and Python integers,
never from the product.  Built once per pair count and shared."""
import random

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
REJECT, ACCEPT, NOT_MEMBER, NOT_ON_CURVE, NOT_IN_SUBGROUP = 0, 1, 2, 3, 4
GT_ONE = (1).to_bytes(32, "big") + bytes(352)
PAIR_COUNTS = (1, 2, 3, 8)


def be(v):
    return int(v).to_bytes(32, "big")


def add_to_field(b, off, delta):
    """the 32-byte big-endian field at `off` of b plus delta, mod p (off the curve for delta != 0 with overwhelming probability; checked by the callers' expectations)"""
    v = (int.from_bytes(b[off:off + 32], "big") + delta) % P
    return b[:off] + be(v) + b[off + 32:]


def twist_point(O, rng):
    """a random point of the twist E'(Fp2): y from a square root of x^3 + 3 / (9 + u) (O.fp2_op 4), gnark byte order"""
    bt = O.fp2_op(2, O.fp2_op(3, (9, 1)), (3, 0))
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        rhs = O.fp2_op(0, O.fp2_op(2, O.fp2_op(5, x), x), bt)
        y = O.fp2_op(4, rhs)
        if y != (0, 0) and O.fp2_op(5, y) == rhs:
            return be(x[1]) + be(x[0]) + be(y[1]) + be(y[0])


def outside_g2(O, rng):
    while True:
        q = twist_point(O, rng)
        if O.g2_subgroup_check(q) == 0:
            return q


_CACHE = {}


def vectors(O, k):
    """[(name, item of 192 k bytes, expected status, expected GT bytes or None)] for items of k pairs"""
    if k in _CACHE:
        return _CACHE[k]
    rng = random.Random(0x9A1B + k)
    g1, g2 = O.g1_gen(), O.g2_gen()
    out = []

    def rand_pairs():
        a = [rng.randrange(1, R) for _ in range(k)]
        b = [rng.randrange(1, R) for _ in range(k)]
        return a, b, [O.g1_mul(g1, x) for x in a], [O.g2_mul(g2, y) for y in b]

    def item(ps, qs):
        return b"".join(p + q for p, q in zip(ps, qs))

    def gt_of(ps, qs, skip=()):
        keep = [j for j in range(k) if j not in skip]
        return O.pairing(b"".join(ps[j] for j in keep), b"".join(qs[j] for j in keep)) if keep else GT_ONE

    # random multiples of the generators: the GT value; the product is not 1
    for t in range(2):
        _, _, ps, qs = rand_pairs()
        gt = gt_of(ps, qs)
        assert gt != GT_ONE
        out.append(("random%d" % t, item(ps, qs), REJECT, gt))
    # a bilinear identity: k - 1 random pairs (a_j G1, b_j G2) and (-(sum a_j b_j) G1, G2) -- for k = 2 the issue's (a G1, b G2), (-ab G1, G2), for more pairs the
    # same padded with further pairs whose contribution the last one cancels; its perturbation: the last scalar plus one
    if k >= 2:
        a, b, ps, qs = rand_pairs()
        s = sum(x * y for x, y in zip(a[:-1], b[:-1])) % R
        ps[-1], qs[-1] = O.g1_mul(g1, (R - s) % R), g2
        out.append(("identity", item(ps, qs), ACCEPT, GT_ONE))
        # the issue's form: (a G1, b G2), (-ab G1, G2), then cancelling pairs (c G1, d G2), (-c G1, d G2), an odd slot taking (0, G2)
        ps2 = [O.g1_mul(g1, a[0]), O.g1_mul(g1, (R - a[0] * b[0] % R) % R)]; qs2 = [O.g2_mul(g2, b[0]), g2]
        while len(ps2) + 2 <= k:
            c, d = rng.randrange(1, R), rng.randrange(1, R)
            ps2 += [O.g1_mul(g1, c), O.g1_mul(g1, R - c)]; qs2 += [O.g2_mul(g2, d)] * 2
        if len(ps2) < k:
            ps2.append(bytes(64)); qs2.append(g2)
        out.append(("identity_padded", item(ps2, qs2), ACCEPT, GT_ONE))
        ps[-1] = O.g1_mul(g1, (R - s + 1) % R)
        out.append(("identity_perturbed", item(ps, qs), REJECT, O.pairing(b"".join(ps), b"".join(qs))))
    # an identity on either side of pair j: the product with that pair omitted
    for j in sorted({0, k - 1}):
        _, _, ps, qs = rand_pairs()
        gt = gt_of(ps, qs, skip=(j,))
        z1 = list(ps); z1[j] = bytes(64)
        out.append(("g1_identity_pair%d" % j, item(z1, qs), ACCEPT if k == 1 else REJECT, gt))
        z2 = list(qs); z2[j] = bytes(128)
        out.append(("g2_identity_pair%d" % j, item(ps, z2), ACCEPT if k == 1 else REJECT, gt))
    # the loader classes in the first and in the last pair
    far = outside_g2(O, rng)
    for j in sorted({0, k - 1}):
        _, _, ps, qs = rand_pairs()
        base = item(ps, qs)
        o = 192 * j
        out.append(("g1_x_ge_p_pair%d" % j, base[:o] + be(P + 5) + base[o + 32:], NOT_MEMBER, None))
        out.append(("g2_y_c0_ge_p_pair%d" % j, base[:o + 160] + be(2 ** 256 - 1) + base[o + 192:], NOT_MEMBER, None))
        out.append(("g1_off_curve_pair%d" % j, add_to_field(base, o + 32, 1), NOT_ON_CURVE, None))
        out.append(("g2_off_curve_pair%d" % j, add_to_field(base, o + 160, 1), NOT_ON_CURVE, None))
        out.append(("g2_outside_subgroup_pair%d" % j, base[:o + 64] + far + base[o + 192:], NOT_IN_SUBGROUP, None))
        # the other point of a pair that contributes 1 is still validated
        out.append(("g1_identity_g2_outside_pair%d" % j, base[:o] + bytes(64) + far + base[o + 192:], NOT_IN_SUBGROUP, None))
        out.append(("g2_identity_g1_off_curve_pair%d" % j, add_to_field(base[:o + 64] + bytes(128) + base[o + 192:], o + 32, 1), NOT_ON_CURVE, None))
        # record order inside a pair: G1 before G2
        out.append(("g1_off_curve_g2_ge_p_pair%d" % j, add_to_field(base[:o + 64] + be(P) + base[o + 96:], o + 32, 1), NOT_ON_CURVE, None))
    if k >= 2:
        _, _, ps, qs = rand_pairs()
        base = item(ps, qs)
        # the two phases: a subgroup failure in pair 0 loses to a curve failure in pair 1
        out.append(("subgroup_pair0_curve_pair1", add_to_field(base[:64] + far + base[192:], 192 + 32, 1), NOT_ON_CURVE, None))
        # phase 1 in record order across pairs: pair 0's G2 off the curve before pair 1's coordinate >= p
        out.append(("curve_pair0_member_pair1", add_to_field(base[:192] + be(P + 1) + base[224:], 160, 1), NOT_ON_CURVE, None))
        out.append(("member_pair0_curve_pair1", add_to_field(base[:96] + be(P) + base[128:], 192 + 32, 1), NOT_MEMBER, None))
    _CACHE[k] = out
    return out


def batch(vecs, n, k, item_stride=None, start=0):
    """n items cycling through vecs from `start`, item_stride bytes apart (the padding bytes are 0xA5): (buffer, expected status bytes, indices into vecs)"""
    stride = 192 * k if item_stride is None else item_stride
    idx = [(start + i) % len(vecs) for i in range(n)]
    buf = b"".join(vecs[j][1] + b"\xa5" * (stride - 192 * k) for j in idx)
    return buf, bytes(vecs[j][2] for j in idx), idx
