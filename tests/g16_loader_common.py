"""Vectors of the Groth16 loader stage, shared by tests/test_g16_loader_cpu.py and tests/test_gpu_g16_loader_values.py (probes bn254_dbg_g16_loader,
bn254_dbg_g16_loader_keys, bn254_dbg_coop12_miller_g16).

Every expectation comes from the CPU oracle (oracle/) and Python integers: L = K_0 + sum (x_j mod r) K_j with O.g1_mul / O.g1_add over the K points decompressed from
the key bytes (the identity handled here: the oracle's group law never sees it), the status byte of a record from the oracle's own verdict on records that differ from
a valid proof in that one point.  Nothing is taken from a run of the code under test, and build_rows() asserts that every row it hands out carries an expectation.

The scalar lists are aimed at the digits the kernels cut a scalar into: 13-bit windows (k_g16_prepare, the cooperative kernels; the top window has 9 bits), comb
columns of 13 teeth x 20 columns (k_g16_comb_digits; tooth 12 exists for columns 0 .. 15 only), bytes (k_g16_msm_partial, k_g16_prepare_keys)."""
import random

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
PENDING, LINF = 0x80, 0x40
NOT_MEMBER, NOT_ON_CURVE = 2, 3
FW_BITS, FW_WINDOWS, FW_MAX = 13, 20, 8191
FW_TOP_BITS = 256 - FW_BITS * (FW_WINDOWS - 1)          # 9
COMB_TEETH, COMB_COLS = 13, 20
SIZES = (257, 65, 64, 63, 1)                            # n of the calls a test cuts its rows into, in turn
VK_K = 292                                              # gnark key bytes: alpha 0, beta 64, gamma 128, delta 224, len(K) at 288, K_i compressed at 292 + 32 i


def be(v):
    return int(v).to_bytes(32, "big")


# ---------------------------------------------------------------------------------------------------------------- digits, as the kernels cut them
def fw_digits(x):
    return [(x >> (FW_BITS * w)) & FW_MAX for w in range(FW_WINDOWS)]


def comb_digits(x):
    """digit of column c: bit t = bit c + 20 t of x (bits from 256 on do not exist)"""
    return [sum(((x >> (c + COMB_COLS * t)) & 1) << t for t in range(COMB_TEETH) if c + COMB_COLS * t < 256) for c in range(COMB_COLS)]


def byte_digits(x):
    """window w = byte 31 - w of the big-endian scalar"""
    return [(x >> (8 * w)) & 0xff for w in range(32)]


# ---------------------------------------------------------------------------------------------------------------- scalar lists
def general_scalars():
    return [0, 1, 2, R - 1, R, R + 1, 2 * R, P, 2 ** 255, 2 ** 254 - 1, 2 ** 256 - 1]


def fw_scalars():
    out = [2 ** 247 - 1]                                                                  # every lower digit 8191, the top window 0
    for w in range(FW_WINDOWS - 1):
        out += [d << (FW_BITS * w) for d in (1, FW_MAX)]
    out += [d << (FW_BITS * (FW_WINDOWS - 1)) for d in (1, 96, 511)]                      # r >> 247 = 96; 2^256 - 1 >> 247 = 511
    out.append(sum(FW_MAX << (FW_BITS * w) for w in range(0, FW_WINDOWS, 2)))             # 8191 in the even windows only
    out.append(sum(FW_MAX << (FW_BITS * w) for w in range(1, FW_WINDOWS, 2)) % 2 ** 256)  # .. in the odd ones only (the top window holds its own maximum, 511)
    return out


def comb_scalars():
    out = [sum(1 << (c + COMB_COLS * t) for t in range(COMB_TEETH) if c + COMB_COLS * t < 256) for c in range(COMB_COLS)]
    out += [1 << (COMB_COLS * t + c) for c in range(COMB_COLS) for t in (0, COMB_TEETH - 1) if COMB_COLS * t + c < 256]
    return out


def byte_scalars():
    out = [v << (8 * j) for j in range(32) for v in (0x01, 0xff)]
    out += [sum(0xff << (8 * j) for j in range(0, 32, 2)), sum(0xff << (8 * j) for j in range(1, 32, 2))]
    return out


def all_scalars():
    """the four lists as one, every value once, in a fixed order"""
    seen, out = set(), []
    for x in general_scalars() + fw_scalars() + comb_scalars() + byte_scalars():
        if x not in seen:
            seen.add(x); out.append(x)
    assert all(0 <= x < 2 ** 256 for x in out)
    return out


# ---------------------------------------------------------------------------------------------------------------- the group, identity = None
def g1_neg(pt):
    return pt[:32] + be((P - int.from_bytes(pt[32:], "big")) % P)


def g1_add(O, a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a == g1_neg(b):
        return None
    r = O.g1_add(a, b)
    assert r != bytes(64)
    return r


def g1_mul(O, pt, k):
    k %= R
    if pt is None or k == 0:
        return None
    r = O.g1_mul(pt, k)
    assert r != bytes(64)
    return r


def key_points(O, vk):
    """K_0 .. K_w of a gnark-format key, through the oracle's decoder"""
    n_k = int.from_bytes(vk[VK_K - 4:VK_K], "big")
    pts = []
    for i in range(n_k):
        st, pt = O.decompress_g1(vk[VK_K + 32 * i:VK_K + 32 * i + 32])
        assert st == O.ACCEPT
        pts.append(pt)
    return pts


def splice_k(O, vk, replace):
    """the key with K_i replaced by the point replace[i] (64 bytes), compressed by the oracle"""
    vk = bytearray(vk)
    for i, pt in replace.items():
        vk[VK_K + 32 * i:VK_K + 32 * i + 32] = O.compress_g1(pt)
    return bytes(vk)


class Row:
    """one proof of a batch: its record, its scalars and what the loader must make of them"""
    __slots__ = ("xs", "rec", "L", "status", "tag")

    def __init__(self, xs, rec, L, status, tag):
        self.xs, self.rec, self.L, self.status, self.tag = xs, rec, L, status, tag

    @property
    def l_bytes(self):
        return be(0) + be(1) if self.L is None else self.L         # the identity is stored as (0, 1)

    def inputs(self, stride=None, fill=0):
        b = b"".join(be(x) for x in self.xs)
        return b if stride is None else b + bytes([fill]) * (stride - len(b))


class KeyCtx:
    """A key's K points, the multiples of them the rows need (each computed once), and random background rows with their sums: a row that differs from a background
    row in a few positions costs one multiplication per position."""

    def __init__(self, O, vk, seed):
        self.O, self.vk, self.k = O, vk, key_points(O, vk)
        self.width = len(self.k) - 1
        self.rng = random.Random(seed)
        self._mul = {}
        self.bgs = []

    def term(self, j, x):
        key = (j, x % R)
        if key not in self._mul:
            self._mul[key] = g1_mul(self.O, self.k[j + 1], x)
        return self._mul[key]

    def L_of(self, xs, n_used=None):
        acc = self.k[0]
        for j, x in enumerate(xs[:self.width if n_used is None else n_used]):
            acc = g1_add(self.O, acc, self.term(j, x))
        return acc

    def background(self, zero_from=None):
        xs = [self.rng.randrange(1, R) for _ in range(self.width)]
        if zero_from is not None:
            xs[zero_from:] = [0] * (self.width - zero_from)
        self.bgs.append((xs, self.L_of(xs)))
        return len(self.bgs) - 1

    def L_override(self, b, over):
        xs, acc = list(self.bgs[b][0]), self.bgs[b][1]
        for j, x in over.items():
            acc = g1_add(self.O, g1_add(self.O, acc, None if self.term(j, xs[j]) is None else g1_neg(self.term(j, xs[j]))), self.term(j, x))
            xs[j] = x
        return xs, acc


class Classes:
    """The records of the loader classes and the status byte the stage must leave for each, from the oracle's verdicts.  base: a valid proof of `vk` for base_xs;
    outside: a record of the same key whose B is on the twist and outside G2 (the generator's class, oracle status NOT_IN_SUBGROUP)."""

    def __init__(self, O, vk, base, base_xs, outside):
        self.O, self.vk, self.base, self.base_in = O, vk, bytes(base), b"".join(be(x) for x in base_xs)
        self.n_in = len(base_xs)
        assert self._verdict(self.base) == O.ACCEPT and self._verdict(outside) == O.ERR_NOT_IN_SUBGROUP
        self._ab, self._c = {}, {}
        b = self.base

        def put(ranges):
            p = bytearray(b)
            for lo, val in ranges:
                p[lo:lo + len(val)] = val
            return bytes(p)

        flip = lambda i: [(i, bytes([b[i] ^ 1]))]
        self.records = [
            ("valid", b),
            ("A = (0, 0)", put([(0, bytes(64))])), ("A.x = p", put([(0, be(P))])), ("A.y = p - 1", put([(32, be(P - 1))])),
            ("B.x.c1 >= p", put([(64, b"\xff" * 32)])), ("B off the twist", put(flip(191))), ("B outside G2", put([(64, outside[64:192])])),
            ("C.x >= p", put([(192, b"\xff" * 32)])), ("C.y >= p", put([(224, b"\xff" * 32)])), ("C off the curve", put(flip(255))),
            ("A.x >= p and C off the curve", put([(0, b"\xff" * 32)] + flip(255))), ("B off the twist and C off the curve", put(flip(191) + flip(255))),
            ("B outside G2 and C off the curve", put([(64, outside[64:192])] + flip(255))), ("B outside G2 and C.x >= p", put([(64, outside[64:192]), (192, b"\xff" * 32)])),
        ]

    def _verdict(self, rec):
        return self.O.groth16_verify(rec, self.vk, [self.base_in[32 * i:32 * i + 32] for i in range(self.n_in)], self.O.MODE_GNARK)

    def status(self, rec):
        """the loader's byte without the identity flag: the oracle's status where A or B decides the proof (a record with this A and B and a good C), else PENDING | the
        oracle's status of a proof whose only defect is this C"""
        O, ab, c = self.O, rec[:192], rec[192:256]
        if ab not in self._ab:
            self._ab[ab] = self._verdict(ab + self.base[192:256])
        if self._ab[ab] in (O.ERR_NOT_MEMBER, O.ERR_NOT_ON_CURVE):
            return self._ab[ab]
        assert self._ab[ab] in (O.ACCEPT, O.REJECT, O.ERR_NOT_IN_SUBGROUP)
        if c not in self._c:
            self._c[c] = self._verdict(self.base[:192] + c)
        assert self._c[c] in (O.ACCEPT, O.REJECT, O.ERR_NOT_MEMBER, O.ERR_NOT_ON_CURVE)
        return PENDING | (self._c[c] if self._c[c] in (O.ERR_NOT_MEMBER, O.ERR_NOT_ON_CURVE) else 0)


def key_bytes(pkg, seed, width):
    """the gnark-format key synth_groth16(seed, width, ..) and synth_groth16_for_inputs(seed, width, ..) make"""
    return pkg.synth_groth16(seed, width, 0)[0]


def make_classes(pkg, O, seed, width):
    """The class records, from the proofs of the key synth_groth16(seed, width, ..) and the generator's own failure classes.  What the loader makes of a record does
    not depend on the key, so the tests attach the records of ONE narrow key to the rows of every key."""
    vk, proofs, inputs, exp = pkg.synth_groth16(seed, width, 24, invalid_every=2, agree=True, threads=4)
    good = next(i for i in range(24) if exp[i] == O.ACCEPT)
    bad_b = next(i for i in range(24) if exp[i] == O.ERR_NOT_IN_SUBGROUP)
    xs = [int.from_bytes(inputs[32 * (width * good + s):32 * (width * good + s) + 32], "big") for s in range(width)]
    cl = Classes(O, vk, proofs[256 * good:256 * good + 256], xs, proofs[256 * bad_b:256 * bad_b + 256])
    gen = [(proofs[256 * i:256 * i + 256], [int.from_bytes(inputs[32 * (width * i + s):32 * (width * i + s) + 32], "big") for s in range(width)], exp[i]) for i in range(24)]
    return vk, cl, gen


def pending(status):
    return (status & PENDING) != 0


def build_rows(ctx, classes, positions, scalars, n_bg=4, zero_bg=False, extra=()):
    """The rows of one key: every scalar in every position of `positions`, the other positions from one of n_bg random background rows (zero_bg: the second half of
    them zero -- the scalar is then the only non-zero digit source of its chunk); then one row per loader class with a background row's scalars, then `extra`
    (lists of (background, overrides, tag)).  Records: the valid base proof except in the class rows."""
    O = ctx.O
    first = len(ctx.bgs)
    for b in range(n_bg):
        ctx.background(zero_from=0 if zero_bg and b >= n_bg // 2 else None)
    rows = []
    base_st = classes.status(classes.base)
    assert base_st == PENDING
    for j in positions:
        for k, x in enumerate(scalars):
            xs, L = ctx.L_override(first + (k + j) % n_bg, {j: x})
            rows.append(Row(xs, classes.base, L, base_st, ("scalar", j, x)))
    for k, (name, rec) in enumerate(classes.records):
        # (every third class row with 2^256 - 1 in the first position, every third with r in the last: decided rows with a scalar >= r exist for the strict flag)
        xs, L = ctx.L_override(first + k % n_bg, {} if k % 3 == 0 else {0: 2 ** 256 - 1} if k % 3 == 1 else {ctx.width - 1: R})
        rows.append(Row(xs, rec, L, classes.status(rec), ("class", name)))
    for b, over, tag in extra:
        xs, L = ctx.L_override(first + b % n_bg, over)
        rows.append(Row(xs, classes.base, L, base_st, tag))
    finish(rows)
    return rows


def finish(rows):
    """the identity flag into the pending bytes; every row carries an expectation"""
    for r in rows:
        if pending(r.status) and r.L is None:
            r.status |= LINF
        assert isinstance(r.status, int) and len(r.rec) == 256 and (r.L is None or len(r.L) == 64) and r.xs is not None, r.tag


def strict_status(row, n_used):
    """BN254_FLAG_STRICT_SCALARS: an input >= r makes the proof NOT_MEMBER ahead of every other outcome; every other row keeps its byte"""
    return NOT_MEMBER if any(x >= R for x in row.xs[:n_used]) else row.status


def cut(rows):
    """the rows in calls of 257, 65, 64, 63, 1, 257, .. proofs (the last call: what is left)"""
    out, i, k = [], 0, 0
    while i < len(rows):
        n = min(SIZES[k % len(SIZES)], len(rows) - i)
        out.append(rows[i:i + n]); i += n; k += 1
    return out


def expected_points(row):
    """A | B | C | L as the probe reads them from the workspace: canonical field values.  A coordinate below p is the record's own 32 bytes.  A pending row can carry a
    coordinate >= p only in C (its error is deferred; such a coordinate of A or B decides the proof): the workspace then holds the field element of that 256-bit
    integer, which reads back as the integer mod p."""
    rec = row.rec
    return b"".join(be(int.from_bytes(rec[o:o + 32], "big") % P) for o in range(0, 256, 32)) + row.l_bytes
