"""Vectors of the batch G1 multi-scalar multiplication (include/bn254_verify.h: bn254_g1_bases_prepare, bn254_g1_msm_batch) for tests/test_g1_msm_cpu.py and
tests/test_gpu_g1_msm_batch.py.  Every point of an item and every shared base is a known multiple of the generator, so the expected status and the expected sum
S = (sum k_t a_t + sum u_t + sum c_j b_j) G1 follow from Python integers and the oracle's g1_mul alone -- never from the product.  Built once per shape and shared;
nothing here calls the library under test."""
import random

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
LAMBDA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd      # the GLV constant: lambda^2 + lambda + 1 = 0 mod r
ACCEPT, NOT_MEMBER, NOT_ON_CURVE = 1, 2, 3
assert (LAMBDA * LAMBDA + LAMBDA + 1) % R == 0

SHAPES = ((1, 0, 0), (0, 2, 0), (0, 1, 0), (0, 0, 1), (2, 1, 0), (3, 1, 2), (16, 4, 16), (0, 0, 16), (16, 0, 0))
SCALARS = (("0", 0), ("1", 1), ("2", 2), ("r_minus_1", R - 1), ("r", R), ("r_plus_1", R + 1), ("2_256_minus_1", 2 ** 256 - 1), ("lambda", LAMBDA),
           ("lambda_minus_1", LAMBDA - 1), ("lambda_plus_1", LAMBDA + 1), ("128bit", 2 ** 127 + 0x1234567), ("129bit", 2 ** 128 + 0x89abcdef))

# every class of vector and the shapes (v, u, s) it exists for
CLASSES = {}
for _n, _k in SCALARS:
    CLASSES["scalar_%s_var" % _n] = lambda v, u, s: v >= 1
    CLASSES["scalar_%s_shared" % _n] = lambda v, u, s: s >= 1
CLASSES.update({
    "identity_var": lambda v, u, s: v >= 1,
    "identity_unit": lambda v, u, s: u >= 1,
    "identity_shared": lambda v, u, s: s >= 2,                 # the base set of a shape with two or more bases holds one identity base
    "cancel_var_unit": lambda v, u, s: v >= 1 and u >= 1,
    "cancel_unit_shared": lambda v, u, s: u >= 1 and s >= 1,
    "same_point_var_unit": lambda v, u, s: v >= 1 and u >= 1,
    "same_point_unit_unit": lambda v, u, s: u >= 2,
    "same_point_var_var": lambda v, u, s: v >= 2,
    "coord_ge_p": lambda v, u, s: v + u >= 1,
    "coord_all_ones": lambda v, u, s: v + u >= 1,
    "off_curve": lambda v, u, s: v + u >= 1,
    "order_range_before_curve_in_point": lambda v, u, s: v + u >= 1,
    "order_strict_beats_curve": lambda v, u, s: v + u >= 1 and v + s >= 1,
    "order_strict_beats_range": lambda v, u, s: v + u >= 1 and v + s >= 1,
    "order_curve_before_later_range": lambda v, u, s: v + u >= 2,
    "order_range_before_later_curve": lambda v, u, s: v + u >= 2,
})
_CACHE = {}


def be(x):
    return int(x).to_bytes(32, "big")


class Vec:
    """One item: its bytes, the decided loader error without / with FLAG_STRICT_SCALARS (None: the item is summed) and the sum as a multiple of G1"""

    def __init__(self, name, rec, scalar, err, strict_err):
        self.name, self.rec, self.scalar, self.err, self.strict_err = name, rec, scalar, err, strict_err

    def status(self, strict=False):
        if strict and self.strict_err is not None:
            return self.strict_err
        return ACCEPT if self.err is None else self.err


def g1_of(O, a):
    """a G1 as 64 bytes (zero: the identity); memoised"""
    a %= R
    memo = _CACHE.setdefault("g1", {0: bytes(64)})
    if a not in memo:
        memo[a] = O.g1_mul(O.g1_gen(), a)
    return memo[a]


def point_pool(O):
    """24 multiples of G1 the items draw their points from"""
    if "pool" not in _CACHE:
        rng = random.Random(0x61A5)
        _CACHE["pool"] = [rng.randrange(2, R) for _ in range(24)]
        for a in _CACHE["pool"]:
            g1_of(O, a)
    return _CACHE["pool"]


def bases(O, n_bases):
    """(multiples b_j, the points as bytes): with two or more bases, base n_bases // 2 is the identity"""
    rng = random.Random(0xBA5E + n_bases)
    bs = [rng.randrange(2, R) for _ in range(n_bases)]
    if n_bases >= 2:
        bs[n_bases // 2] = 0
    return bs, b"".join(g1_of(O, b) for b in bs)


def encode(O, var, unit, shared):
    """var: [(a, k)] point a G1 and scalar k as encoded; unit: [a]; shared: [c]"""
    return b"".join(g1_of(O, a) + be(k) for a, k in var) + b"".join(g1_of(O, a) for a in unit) + b"".join(be(c) for c in shared)


def vectors(O, shape):
    """(base multiples, base points, [Vec]) of a shape: every class of CLASSES that exists for it, an error item between two valid ones (positions 1 .. 3), and valid
    items enough that more than half of the list is summed to a point other than the identity, with and without FLAG_STRICT_SCALARS"""
    if shape in _CACHE:
        return _CACHE[shape]
    v, u, s = shape
    rng = random.Random(0x6D5301 + 1000 * v + 100 * u + s)
    pool = point_pool(O)
    bs, bpts = bases(O, s)
    live = [j for j in range(s) if bs[j] != 0]
    out = []

    def rand_terms():
        return ([(rng.choice(pool), rng.randrange(1, R)) for _ in range(v)], [rng.choice(pool) for _ in range(u)], [rng.randrange(1, R) for _ in range(s)])

    def total(var, unit, shared):
        return (sum(a * k for a, k in var) + sum(unit) + sum(c * b for c, b in zip(shared, bs))) % R

    def emit(name, var, unit, shared, rec=None, err=None, strict_err=None):
        if strict_err is None and any(k >= R for _, k in var) or any(c >= R for c in shared):
            strict_err = NOT_MEMBER
        out.append(Vec(name, encode(O, var, unit, shared) if rec is None else rec, None if err is not None else total(var, unit, shared), err, strict_err))

    def point_off(t):
        """offset of the t-th point of an item in record order"""
        return 96 * t if t < v else 96 * v + 64 * (t - v)

    def put(rec, off, field):
        return rec[:off] + field + rec[off + 32:]

    def bump(rec, off):
        return put(rec, off, be((int.from_bytes(rec[off:off + 32], "big") + 1) % P))

    def first_scalar_off():
        return 64 if v else 96 * v + 64 * u

    emit("valid_first", *rand_terms())
    if v + u >= 1:      # an error item between two valid ones
        var, unit, shared = rand_terms()
        emit("error_between_valid", var, unit, shared, rec=bump(encode(O, var, unit, shared), point_off(0) + 32), err=NOT_ON_CURVE)
    else:               # a shape without points of its own has only the strict error
        var, unit, shared = rand_terms()
        emit("error_between_valid", var, unit, [shared[0] + R] + shared[1:])
    emit("valid_third", *rand_terms())
    for name, k in SCALARS:
        if v:
            var, unit, shared = rand_terms()
            emit("scalar_%s_var" % name, [(var[0][0], k)] + var[1:], unit, shared)
        if s:
            var, unit, shared = rand_terms()
            j = live[0]
            emit("scalar_%s_shared" % name, var, unit, shared[:j] + [k] + shared[j + 1:])
    if v:
        var, unit, shared = rand_terms()
        emit("identity_var", [(0, var[0][1])] + var[1:], unit, shared)
    if u:
        var, unit, shared = rand_terms()
        emit("identity_unit", var, [0] + unit[1:], shared)
    if s >= 2:
        var, unit, shared = rand_terms()
        j = bs.index(0)
        emit("identity_shared", var, unit, shared[:j] + [2 ** 256 - 1 - R * 5] + shared[j + 1:])
    # P and -P across kinds: everything else of the item contributes nothing, so the sum is the identity
    if v and u:
        a, k = rng.choice(pool), rng.randrange(1, R)
        emit("cancel_var_unit", [(a, k)] + [(0, rng.randrange(R)) for _ in range(v - 1)], [-(a * k) % R] + [0] * (u - 1), [0] * s)
        assert out[-1].scalar == 0
    if u and s:
        j, c = live[-1], rng.randrange(1, R)
        emit("cancel_unit_shared", [(rng.choice(pool), 0) for _ in range(v)], [0] * (u - 1) + [-(c * bs[j]) % R], [c if q == j else 0 for q in range(s)])
        assert out[-1].scalar == 0
    # the same point in two positions: the doubling case of the complete formulas
    if v and u:
        var, unit, shared = rand_terms()
        emit("same_point_var_unit", [(var[0][0], 1)] + [(0, 0)] * (v - 1), [var[0][0]] + [0] * (u - 1), [0] * s)
    if u >= 2:
        var, unit, shared = rand_terms()
        emit("same_point_unit_unit", [(a, 0) for a, _ in var], [unit[0], unit[0]] + [0] * (u - 2), [0] * s)
    if v >= 2:
        var, unit, shared = rand_terms()
        emit("same_point_var_var", [var[0], var[0]] + [(0, 0)] * (v - 2), [0] * u, [0] * s)
    if v + u >= 1:
        var, unit, shared = rand_terms()
        good = encode(O, var, unit, shared)
        last = v + u - 1
        emit("coord_ge_p", var, unit, shared, rec=put(good, point_off(0), be(P + 3)), err=NOT_MEMBER)
        emit("coord_all_ones", var, unit, shared, rec=put(good, point_off(last) + 32, be(2 ** 256 - 1)), err=NOT_MEMBER)
        emit("off_curve", var, unit, shared, rec=bump(good, point_off(last) + 32), err=NOT_ON_CURVE)
        # inside one point the range check comes first
        emit("order_range_before_curve_in_point", var, unit, shared, rec=put(bump(good, point_off(0)), point_off(0) + 32, be(P + 9)), err=NOT_MEMBER)
        if v + s >= 1:
            off = first_scalar_off()
            k = int.from_bytes(good[off:off + 32], "big") + R
            emit("order_strict_beats_curve", var, unit, shared, rec=put(bump(good, point_off(0) + 32), off, be(k)), err=NOT_ON_CURVE, strict_err=NOT_MEMBER)
            emit("order_strict_beats_range", var, unit, shared, rec=put(put(good, point_off(0), be(P)), off, be(k)), err=NOT_MEMBER, strict_err=NOT_MEMBER)
        if v + u >= 2:
            emit("order_curve_before_later_range", var, unit, shared, rec=put(bump(good, point_off(0) + 32), point_off(last), be(P)), err=NOT_ON_CURVE)
            emit("order_range_before_later_curve", var, unit, shared, rec=bump(put(good, point_off(0) + 32, be(P + 1)), point_off(last) + 32), err=NOT_MEMBER)
    weak = sum(1 for x in out if x.status(True) != ACCEPT or x.scalar == 0)
    for t in range(weak + 2):
        emit("fill%d" % t, *rand_terms())
    assert len({x.name for x in out}) == len(out)
    for name, exists in CLASSES.items():
        assert (name in {x.name for x in out}) == bool(exists(v, u, s)), (shape, name)
    _CACHE[shape] = (bs, bpts, out)
    return _CACHE[shape]


def batch(vecs, n, item_len, stride=None, start=0, step=1):
    """n items cycling through vecs from `start` in steps of `step`: (buffer at `stride`, the Vec of each item)"""
    stride = item_len if stride is None else stride
    idx = [(start + i * step) % len(vecs) for i in range(n)]
    return b"".join(vecs[j].rec + b"\xa5" * (stride - item_len) for j in idx), [vecs[j] for j in idx]


def expected(O, members, strict=False):
    """(out bytes, status bytes) as the definition gives them: zero bytes for the identity and for an item that ends in an error"""
    st = bytes(x.status(strict) for x in members)
    return b"".join(g1_of(O, x.scalar) if c == ACCEPT else bytes(64) for x, c in zip(members, st)), st


def summed_share(O, members, strict=False):
    """share of the items that end ACCEPT with a result other than the identity"""
    out, st = expected(O, members, strict)
    return sum(1 for i, c in enumerate(st) if c == ACCEPT and out[64 * i:64 * i + 64] != bytes(64)) / max(len(members), 1)


def pool257(O, shape):
    """257 valid and invalid items of a shape for the large batches (results from the oracle, once): every eighth item carries a loader error when the shape has a point"""
    key = ("pool257", shape)
    if key not in _CACHE:
        v, u, s = shape
        rng = random.Random(0x257 + 100 * v + 10 * u + s)
        pool = point_pool(O)
        bs, bpts = bases(O, s)
        out = []
        for t in range(257):
            var = [(rng.choice(pool), rng.randrange(2 ** 256 if t % 5 == 0 else R)) for _ in range(v)]
            unit = [rng.choice(pool) for _ in range(u)]
            shared = [rng.randrange(R) for _ in range(s)]
            rec = encode(O, var, unit, shared)
            strict_err = NOT_MEMBER if any(k >= R for _, k in var) else None
            if t % 8 == 3 and v + u:
                off = (96 * (v - 1) if v else 64 * (u - 1)) + 32
                rec = rec[:off] + be((int.from_bytes(rec[off:off + 32], "big") + 1) % P) + rec[off + 32:]
                out.append(Vec("bad%d" % t, rec, None, NOT_ON_CURVE, strict_err))
            else:
                out.append(Vec("ok%d" % t, rec, (sum(a * k for a, k in var) + sum(unit) + sum(c * b for c, b in zip(shared, bs))) % R, None, strict_err))
        _CACHE[key] = (bs, bpts, out)
    return _CACHE[key]
