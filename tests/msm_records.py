"""Inputs and expected sums of the G1 multi-scalar multiplications of the PlonK path (csrc/bn254_msm.h, csrc/bn254_k_msm.hip), shared by the CPU tests
(tests/test_msm_rows.py, tests/test_msm_records_cpu.py: the host stand-in hs_msm_rows_joint) and the GPU test (tests/test_gpu_g1_msm_values.py: the probes
bn254_dbg_g1_msm, bn254_dbg_g1_sum_rows, bn254_dbg_plonk_group_sums).

Expected values come from the oracle (O.g1_mul, O.g1_add) and Python integers alone.  The one thing taken from the product is the GLV decomposition of a scalar
(bn254_dbg_glv_decompose), and only as an INPUT: the expected point of a variable term is k P by the oracle, whatever halves the decomposition returned.  Where a
test writes the halves itself the expected scalar is +-k1 +- k2 lambda mod r with the lambda computed here."""
import ctypes as C
import random
import struct

import fp12_digits as D

P = D.P
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ID = bytes(64)                       # how the tests write the identity (never sent to a kernel as a point)
PENDING, LINF, LINF2 = 0x80, 0x40, 0x20
ACCEPT, REJECT, NOT_ON_CURVE = 1, 0, 3
FW_BITS, FW_WINDOWS = 13, 20         # csrc/bn254_fw.h: the window tables of the key-side points
MAX_ROWS = 32                        # csrc/bn254_msm.h MSM_MAX_ROWS
SPLIT, UNSPLIT, JOINT = 0, 1, 2      # info[4] of bn254_dbg_g1_msm


def be(v):
    return int(v).to_bytes(32, "big")


def neg(pt):
    return ID if pt == ID else pt[:32] + be(P - int.from_bytes(pt[32:], "big"))


def add(O, a, b):
    """a + b with the identity as ID on either side and as the result"""
    if a == ID:
        return b
    if b == ID:
        return a
    if a == neg(b):
        return ID
    return O.g1_add(a, b)


def mul(O, pt, k):
    k %= R
    return ID if k == 0 or pt == ID else O.g1_mul(pt, k)


_LAM = {}


def lam_beta(O):
    """(lambda, beta): beta a primitive cube root of 1 in Fp, lambda the root of x^2 + x + 1 in Fr with lambda G = (beta x_G, y_G) by the oracle.  Of the two such
    pairs (lambda, beta) and (lambda^2, beta^2) this is the one with lambda < 2^192: the endomorphism the GLV halves of csrc/bn254_plonk.hpp refer to."""
    if not _LAM:
        beta = next(b for b in (pow(g, (P - 1) // 3, P) for g in range(2, 64)) if b != 1)
        lam = next(x for x in (pow(g, (R - 1) // 3, R) for g in range(2, 64)) if x != 1)
        assert (beta * beta + beta + 1) % P == 0 and (lam * lam + lam + 1) % R == 0
        lam = min(lam, lam * lam % R)
        assert lam < 1 << 192
        g = O.g1_gen()
        x = int.from_bytes(g[:32], "big")
        got = O.g1_mul(g, lam)
        for b in (beta, beta * beta % P):
            if got == be(b * x % P) + g[32:]:
                _LAM["v"] = (lam, b)
        assert "v" in _LAM, "lambda G is not (beta x, y) for either cube root"
    return _LAM["v"]


def glv(L, k):
    """the halves the product's decomposition gives for k: (|k1|, |k2|, flag bits 2 / 4 for their signs)"""
    k1, k2 = (C.c_uint8 * 16)(), (C.c_uint8 * 16)()
    n1, n2 = C.c_int(), C.c_int()
    assert L.bn254_dbg_glv_decompose(int(k % R).to_bytes(32, "big"), k1, k2, C.byref(n1), C.byref(n2)) == 0
    return bytes(k1), bytes(k2), (2 if n1.value else 0) | (4 if n2.value else 0)


def halves_scalar(O, k1, k2, neg1, neg2):
    lam, _ = lam_beta(O)
    return ((-k1 if neg1 else k1) + (-k2 if neg2 else k2) * lam) % R


def shape_list(sums):
    """sums: [(var terms, unit terms, [(fixed term, table)])] -> the int encoding of hs_msm_rows_joint / bn254_dbg_g1_msm"""
    out = [len(sums)]
    for v, u, f in sums:
        out += [len(v), len(u), len(f)]
    for v, u, f in sums:
        out += list(v) + list(u) + [t for t, _ in f] + [b for _, b in f]
    return out


def shape_ints(sums):
    out = shape_list(sums)
    return (C.c_int * len(out))(*out)


def n_tables(sums):
    return 1 + max([b for _, _, f in sums for _, b in f] + [0])


def random_bases(O, rng, count):
    g = O.g1_gen()
    return [O.g1_mul(g, rng.randrange(1, R)) for _ in range(count)]


def junk_point(rng):
    """64 bytes below p in both halves that are NOT a curve point: what sits under an identity flag"""
    while True:
        x, y = rng.randrange(1, P), rng.randrange(1, P)
        if (y * y - x * x * x - 3) % P:
            return be(x) + be(y)


def build_item(L, O, rng, sums, n_terms, bases, zero_scalar_terms=(), identity_terms=(), spec=None):
    """One item: n_terms records of 129 bytes and the expected point of every sum (ID: the identity).
    Without `spec` every term is random, as tests/test_msm_rows.py always drew them: a random point, a scalar from a few classes; zero_scalar_terms get the scalar 0,
    identity_terms (variable terms) the identity flag on a zero point.  spec: {term: {..}} overrides --
      variable   p (point), k (scalar, decomposed by the product) or halves = (k1, k2, neg1, neg2) written as given; identity = True with junk (64 bytes under the flag)
      unit       p, neg, identity, junk
      fixed      k"""
    g = O.g1_gen()
    spec = spec or {}
    kinds = {}
    for s, (v, u, f) in enumerate(sums):
        for t in v: kinds[t] = ("var", s, None)
        for t in u: kinds[t] = ("unit", s, None)
        for t, b in f: kinds[t] = ("fixed", s, b)
    acc = [ID] * len(sums)
    recs = []
    for t in range(n_terms):
        kind, s, b = kinds.get(t, ("none", 0, None))
        sp = spec.get(t, {})
        p = O.g1_mul(g, rng.randrange(1, R))
        k = 0 if t in zero_scalar_terms else rng.choice([rng.randrange(R), rng.randrange(1 << 64), R - 1, 1, rng.randrange(R)])
        p = sp.get("p", p)
        k = sp.get("k", k)
        if kind == "var":
            if "halves" in sp:
                h1, h2, n1, n2 = sp["halves"]
                k1, k2, fl = h1.to_bytes(16, "big"), h2.to_bytes(16, "big"), (2 if n1 else 0) | (4 if n2 else 0)
                k = halves_scalar(O, h1, h2, n1, n2)
            else:
                k1, k2, fl = glv(L, k)
            if t in identity_terms or sp.get("identity"):
                recs.append(sp.get("junk", ID) + k1 + k2 + bytes(32) + bytes([fl | 1]))
            else:
                recs.append(p + k1 + k2 + bytes(32) + bytes([fl]))
                acc[s] = add(O, acc[s], mul(O, p, k))
        elif kind == "unit":
            ng = sp["neg"] if "neg" in sp else rng.randrange(2)
            if sp.get("identity"):
                recs.append(sp.get("junk", ID) + bytes(32) + bytes(32) + bytes([(2 if ng else 0) | 1]))
            else:
                recs.append(p + bytes(32) + bytes(32) + bytes([2 if ng else 0]))
                acc[s] = add(O, acc[s], neg(p) if ng else p)
        elif kind == "fixed":
            recs.append(bytes(64) + bytes(32) + (k % R).to_bytes(32, "little") + bytes([0]))
            acc[s] = add(O, acc[s], mul(O, bases[b], k))
        else:
            recs.append(bytes(129))
    return recs, acc


def build_items(L, O, rng, sums, n_terms, n, bases=None, zero_scalar_terms=(), identity_terms=(), spec_of=None, bases_of=None):
    """n items: (records: n x n_terms x 129 bytes, bases, want[i][s]).  spec_of(i) -> the spec of item i (None: random); bases_of(i): the bases item i's fixed
    terms multiply (a batch over a key list), default the one list."""
    if bases is None:
        bases = random_bases(O, rng, n_tables(sums))
    recs, want = [], []
    for i in range(n):
        while True:                    # every item of a call holds different values: a draw that repeats an earlier item (two terms, scalars 1 and r - 1) is made again
            r, w = build_item(L, O, rng, sums, n_terms, bases_of(i) if bases_of else bases, zero_scalar_terms, identity_terms, spec_of(i) if spec_of else None)
            if b"".join(r) not in recs:
                break
        recs.append(b"".join(r))
        want.append(w)
    return b"".join(recs), bases, want


def host_sums(hostsim, sums, n_terms, records, bases, n, n_pad, budget, joint_g):
    """every item through tests/hostsim's hs_msm_rows_joint (the rows of csrc/bn254_msm.h on the CPU, bound tracker on): (sums[i][s], info of the plan)"""
    sh = shape_ints(sums)
    bb = b"".join(bases)
    got, info = [], (C.c_int * 5)()
    for i in range(n):
        out = (C.c_uint8 * (64 * len(sums)))()
        assert hostsim.hs_msm_rows_joint(out, info, sh, records[129 * n_terms * i:129 * n_terms * (i + 1)], bb, n_pad, budget, joint_g) == 1
        o = bytes(out)
        got.append([o[64 * s:64 * s + 64] for s in range(len(sums))])
    return got, list(info)


# ---------------------------------------------------------------------------------------------------------------- the shapes
Q = 1
S1 = [([0, Q + 6, Q + 7, Q + 8, Q + 9], [], [(Q + i, i) for i in range(6)])]                                  # the first launch of a key with one BSB22 commitment
S2 = [([0, 1, 2, 3, 6 + Q, 8 + Q, 9 + Q], [], [(4, 6), (5, 7), (6, 9), (7 + Q, 8)]), ([11 + Q], [10 + Q], [])]      # the second: P0 and P1 of the KZG check
T1, T2 = 10 + Q, 12 + Q
# the second launch of a key with EIGHT commitments (csrc/bn254_plonk.hpp::plonk_msm2_shape): eleven fixed terms, the most table indices a key has (renumbered 0 .. 10)
S2_Q8 = [([0, 1, 2, 3, 14, 16, 17], [], [(4 + i, i) for i in range(10)] + [(15, 10)]), ([19], [18], [])]
T2_Q8 = 20
FIXED_ONLY = [([], [], [(0, 0), (1, 1)])]
UNIT_ONLY = [([], [0, 1], [])]
EMPTY_SECOND = [([0], [], []), ([], [], [])]
SEVEN_FIXED = [([0], [1], [(2 + i, i % 3) for i in range(7)])]


def plan_cases():
    """(name, sums, n_terms, n, lane budget, joint_g, expected form): the plan forms and the item counts of the first group of tests/test_gpu_g1_msm_values.py.
    n = 70: n_pad = 128, the second wavefront of every row has 58 dead lanes.  Budget 65 536 splits every variable term over two rows, budget 64 does not."""
    out = []
    for nm, sums, nt in (("s1", S1, T1), ("s2", S2, T2)):
        out.append((nm + "-split", sums, nt, 70, 65536, 0, SPLIT))
        out.append((nm + "-unsplit", sums, nt, 70, 64, 0, UNSPLIT))
        for g in (2, 4, 8):
            out.append(("%s-joint%d" % (nm, g), sums, nt, 70, 64, g, JOINT))
    out.append(("fixed-only", FIXED_ONLY, 2, 70, 65536, 0, UNSPLIT))
    out.append(("unit-only", UNIT_ONLY, 2, 70, 65536, 0, UNSPLIT))
    out.append(("empty-second", EMPTY_SECOND, 1, 70, 65536, 0, SPLIT))
    out.append(("seven-fixed-split", SEVEN_FIXED, 9, 70, 65536, 0, SPLIT))
    out.append(("seven-fixed-unsplit", SEVEN_FIXED, 9, 70, 64, 0, UNSPLIT))
    out.append(("s2q8-split", S2_Q8, T2_Q8, 70, 65536, 0, SPLIT))
    out.append(("s2q8-joint4", S2_Q8, T2_Q8, 70, 64, 4, JOINT))
    for n in (1, 64, 129):
        out.append(("s1-n%d" % n, S1, T1, n, 65536, 0, SPLIT))
    return out


# ---------------------------------------------------------------------------------------------------------------- chosen scalars
def two_bit_halves(digit, where):
    """a 128-bit half from its 64 two-bit digits: all `digit` (where = "all"), or zero but the lowest / the highest"""
    if where == "all":
        return sum(digit << (2 * j) for j in range(64))
    return digit << (0 if where == "low" else 126)


def var_scalar_specs(O):
    """what a variable term is multiplied by, one entry per item: ("k", scalar) through the decomposition, or ("halves", (k1, k2, neg1, neg2)) as given"""
    lam, _ = lam_beta(O)
    top = (1 << 127) - 1
    out = [("k", 0), ("k", 1), ("k", R - 1), ("k", lam), ("k", lam * lam % R), ("k", (1 << 64) - 1), ("k", 0x0123456789abcdef), ("k", 1 << 63),
           ("halves", (1, 0, 0, 0)), ("halves", (0, 1, 0, 0)), ("halves", (1, 1, 1, 1)), ("halves", (0, 1, 0, 1)),
           ("halves", (top, top, 0, 0)), ("halves", (top, top, 1, 0)), ("halves", (1 << 126, top, 0, 1)), ("halves", (top, 1 << 126, 1, 1)),
           ("halves", ((1 << 127) | 1, 3 << 126, 0, 0))]                    # the top bit itself: the walk takes all 128 positions, whatever the decomposition returns
    for d in (3, 2, 1):
        for where in ("all", "low", "high"):
            h = two_bit_halves(d, where)
            out += [("halves", (h, h, 0, 1)), ("halves", (h, 0, 1, 0)), ("halves", (0, h, 0, 0))]
    out.append(("halves", (two_bit_halves(3, "low"), two_bit_halves(3, "high"), 0, 0)))
    out.append(("halves", (two_bit_halves(1, "high"), two_bit_halves(2, "low"), 1, 1)))
    return out


def fixed_scalar_specs():
    """scalars of a fixed term: 0, 1, every 13-bit digit 8191 as far as that stays below r, r - 1 (the short top window), one non-zero digit per window in turn (every
    word-straddling shift of the digit extraction), the last entry of one window at a time"""
    out = [0, 1, (1 << 247) - 1, R - 1, R - 2, (1 << 253) + 1]
    assert (1 << 247) - 1 < R
    for w in range(FW_WINDOWS):
        d = (0x1555 ^ (w * 0x3b1)) & 0x1fff or 1
        if w == FW_WINDOWS - 1:
            d &= 0x3f                                   # the top window holds bits 247 .. 253 of a scalar below r
            d = d or 1
        k = d << (FW_BITS * w)
        assert k < R
        out.append(k)
    for w in range(FW_WINDOWS - 1):
        out.append(8191 << (FW_BITS * w))
    return out


# ---------------------------------------------------------------------------------------------------------------- small multiples of G (sum-only and group-sum probes)
class Multiples:
    """m G for |m| <= limit, built once by repeated O.g1_add; -m G is (x, p - y); 0 is ID"""
    def __init__(self, O, limit=4096):
        g = O.g1_gen()
        self.limit = limit
        self.pos = [ID, g]
        for _ in range(limit - 1):
            self.pos.append(O.g1_add(self.pos[-1], g))

    def __call__(self, m):
        assert abs(m) <= self.limit, m
        return self.pos[m] if m >= 0 else neg(self.pos[-m])

    def xy(self, m):
        pt = self(m)
        return int.from_bytes(pt[:32], "big"), int.from_bytes(pt[32:], "big")


def proj_bytes(x, y, z):
    return be(x % P) + be(y % P) + be(z % P)


def proj_row(tab, m, rng=None, identity_y=1):
    """m G as a projective row of format 0 (96 bytes): Z = 1, or the coordinates scaled by a random factor; m = 0: (0 : identity_y : 0)"""
    if m == 0:
        return proj_bytes(0, identity_y, 0)
    x, y = tab.xy(m)
    z = rng.randrange(2, P) if rng else 1
    return proj_bytes(x * z, y * z, z)


def rep_digits(value, shift):
    """the Montgomery residue of the field value as the representative m + shift p: nine balanced digits"""
    return D.encode(D.mont(value) + shift * P)


def raw_row(coords):
    """three digit lists (X, Y, Z) -> the 108 bytes of a row in format 1"""
    return b"".join(struct.pack("<9i", *d) for d in coords)


def extreme_rep(value, high):
    """the largest (smallest) representative of the value inside +-3 p"""
    m = D.mont(value)
    return D.encode(m + 2 * P if high else m - 3 * P)


def pattern_point(kind, rng):
    """a curve point whose X has the digit pattern `kind` of fp12_digits.pattern in its eight low digits: the top digit is varied until x^3 + 3 is a square.
    Returns (X digits, x, y) with y from the exponent (p + 1) / 4 (p = 3 mod 4)."""
    lim = (3 * P) >> (D.LB * (D.NL - 1))
    for _ in range(4096):
        top = rng.randrange(-lim, lim + 1)
        d = D.pattern(kind, top)
        if not D.in_contract(d, 3):
            continue
        x = D.field_value(d)
        rhs = (x * x * x + 3) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return d, x, y
    raise AssertionError("no top digit puts the pattern on the curve")


# ---------------------------------------------------------------------------------------------------------------- the cases of the first group
STATUS_CYCLE = [PENDING, PENDING | 3, ACCEPT, REJECT, NOT_ON_CURVE]      # PENDING | 3: a deferred code rides in the low bits
POINT_KINDS = ["idflags", "cancel0", "double", "base-opp", "cancel1", "both", "random"]
FLAG_WORD = {8: "cancel0", 9: "cancel1", 10: "both", 11: "cancel0"}      # items 8 .. 11: one status word, every byte of it pending and flagged
KEY_GRANULES = [2, 0, 1, 0]


def status_in(n):
    return bytes((PENDING | (3 if i & 1 else 0)) if i in FLAG_WORD else STATUS_CYCLE[i % 5] for i in range(n))


def point_kind(i):
    return FLAG_WORD.get(i, POINT_KINDS[i % len(POINT_KINDS)])


def _point_spec(O, rng, bases, kind, i):
    """the second launch (S2: sum 0 = variable terms 0 1 2 3 7 9 10 + fixed terms 4 5 6 8, sum 1 = unit term 11 + variable term 12) with the points where the
    complete formulas have their exceptional cases"""
    g = O.g1_gen()
    pt = O.g1_mul(g, rng.randrange(1, R))
    k = rng.randrange(1, R)
    sp = {}
    quiet0 = {t: {"identity": True, "junk": junk_point(rng)} for t in (2, 3, 7, 9, 10)}
    quiet0.update({t: {"k": 0} for t in (4, 5, 6, 8)})
    if kind == "idflags":              # the flag on a variable term and on the unit term, junk under it: neither may count
        sp = {1: {"identity": True, "junk": junk_point(rng)}, 11: {"identity": True, "junk": junk_point(rng)}}
    elif kind == "double":             # the same point with the same scalar twice: the row sum doubles
        sp = {0: {"p": pt, "k": k}, 1: {"p": pt, "k": k}}
    elif kind == "base-opp":           # a variable term on the base of a fixed term, scalars opposite: the fixed windows' row meets its negative
        sp = {0: {"p": bases[6], "k": R - k}, 4: {"k": k}}
    if kind in ("cancel0", "both"):    # k P - k P and nothing else: sum 0 is the identity
        sp.update(quiet0)
        sp.update({0: {"p": pt, "k": k}, 1: {"p": pt, "k": R - k}})
    if kind in ("cancel1", "both"):    # P (the unit term) and (r - 1) P: sum 1 is the identity
        q = O.g1_mul(g, rng.randrange(1, R)) if i & 1 else pt
        sp.update({11: {"p": q, "neg": 0}, 12: {"p": q, "k": R - 1}})
    return sp


def value_cases():
    """(name, sums, n_terms, n, lane budget, joint_g, form, what): the chosen scalars and points, each in every plan form"""
    out = []
    for nm, budget, g, form in (("split", 65536, 0, SPLIT), ("unsplit", 64, 0, UNSPLIT), ("joint4", 64, 4, JOINT)):
        out.append(("var-scalars-" + nm, S1, T1, 70, budget, g, form, "var-scalars"))
        out.append(("points-" + nm, S2, T2, 70, budget, g, form, "points"))
    out.append(("fixed-scalars-split", S1, T1, 70, 65536, 0, SPLIT, "fixed-scalars"))
    out.append(("fixed-scalars-unsplit", S1, T1, 70, 64, 0, UNSPLIT, "fixed-scalars"))
    out.append(("joint-all-identity", S1, T1, 70, 64, 8, JOINT, "all-identity"))
    out.append(("keys", S1, T1, 200, 65536, 0, SPLIT, "keys"))
    return out


def all_cases():
    return [c + ("random",) for c in plan_cases()] + value_cases()


def case_names():
    return [c[0] for c in all_cases()]


_CASES = {}


def build_case(L, O, name):
    """The inputs and the oracle's sums of one case, built once per process and never modified: a dict with sums, n_terms, n, budget, joint_g, form, records,
    bases (one list, or one per key with granule_key), want[i][s]."""
    if name in _CASES:
        return _CASES[name]
    _, sums, n_terms, n, budget, joint_g, form, what = next(c for c in all_cases() if c[0] == name)
    rng = random.Random("msm-case-" + name)
    case = {"name": name, "sums": sums, "n_terms": n_terms, "n": n, "budget": budget, "joint_g": joint_g, "form": form, "what": what, "granule_key": None}
    bases = random_bases(O, rng, n_tables(sums))
    spec_of, bases_of, ident = None, None, ()
    if what == "var-scalars":
        specs = var_scalar_specs(O)
        var = sums[0][0]
        spec_of = lambda i: {t: dict([specs[(i + 7 * j) % len(specs)]]) for j, t in enumerate(var)}
    elif what == "fixed-scalars":
        fs = fixed_scalar_specs()
        spec_of = lambda i: {t: {"k": fs[(i + 5 * j) % len(fs)]} for j, (t, _) in enumerate(sums[0][2])}
    elif what == "points":
        spec_of = lambda i: _point_spec(O, rng, bases, point_kind(i), i)
    elif what == "all-identity":       # every term of the one joint group flagged, junk under every flag: the sum is what the fixed terms give
        spec_of = lambda i: {t: {"identity": True, "junk": junk_point(rng)} for t in sums[0][0]}
    elif what == "keys":
        key_bases = [bases, random_bases(O, rng, len(bases)), random_bases(O, rng, len(bases))]
        case["granule_key"] = KEY_GRANULES
        case["key_bases"] = key_bases
        bases_of = lambda i: key_bases[KEY_GRANULES[i // 64]]
    records, _, want = build_items(L, O, rng, sums, n_terms, n, bases=bases, spec_of=spec_of, bases_of=bases_of)
    assert len({records[129 * n_terms * i:129 * n_terms * (i + 1)] for i in range(n)}) == n, "two items of a call hold the same values"
    case.update(records=records, bases=bases, want=want)
    _CASES[name] = case
    return case


def item_bases(case, i):
    return case["key_bases"][case["granule_key"][i // 64]] if case["granule_key"] else case["bases"]
