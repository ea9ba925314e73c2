"""Value-level GPU tests of the twelve-lane (cooperative) kernels of csrc/bn254_coop12.hip, of the lane kernels on edge operands and chosen
representatives, and of every compare that decides a verdict.  Everything is bit-exact: the expected values come from the CPU oracle (oracle/) and from Python
integers, never from another run of the code under test.  n = 13 for the cooperative probes (wavefronts of 5, 5 and 3 proofs: shadow lanes and dead groups
take part), n = 70 for the lane probes (two wavefronts); every proof of a call holds a different value."""
import ctypes as C
import random

import pytest

import fp12_digits as D

pytestmark = pytest.mark.gpu
P = D.P
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NC, NL_ = 13, 70
ACCEPT, REJECT = 1, 0
# bn254_dbg_coop12_op (include/bn254_verify.h)
MUL, MUL_CONJ_B, MUL_CONJ_A, SQR, CYCLO_N, FROB, INV, CONJ, LINE_FP, LINE_FP_KEEP, LINE_FP2, FINAL_EXP = range(12)
# oracle fp12_op
O_MUL, O_SQR, O_INV, O_FROB1, O_FROB2, O_FROB3, O_CYCLO, O_CONJ = range(8)
LONGEST_RUN = 7   # of Granger-Scott squarings between two products of the exponentiation by u (the zeros between -7 and 5 in BN_U_W4, csrc/bn254_constants.h)


def be(v):
    return int(v).to_bytes(32, "big")


def _chk(L, rc):
    assert rc == 0, L.bn254_last_error()


@pytest.fixture(scope="module")
def L(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    lib = pkg.lib()
    lib.bn254_dbg_coop12_op.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bn254_dbg_fp12_op_fmt.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int]
    lib.bn254_dbg_verdict.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    lib.bn254_dbg_coop12_miller_fixed.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.bn254_dbg_coop12_miller_g16.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def _size(fmt):
    return 432 if fmt else 384


def coop_op(L, op, a, b, n, fmt_in=0, fmt_out=0, arg=0):
    assert len(a) == n * _size(fmt_in) and (b is None or len(b) == n * _size(fmt_in))
    out = (C.c_uint8 * (n * _size(fmt_out)))()
    _chk(L, L.bn254_dbg_coop12_op(op, a, b, out, n, fmt_in, fmt_out, arg, 0))
    out = bytes(out)
    return [out[_size(fmt_out) * i:_size(fmt_out) * (i + 1)] for i in range(n)]


def lane_op(L, op, a, b, n, fmt_in=0, fmt_out=0):
    assert len(a) == n * _size(fmt_in) and (b is None or len(b) == n * _size(fmt_in))
    out = (C.c_uint8 * (n * _size(fmt_out)))()
    _chk(L, L.bn254_dbg_fp12_op_fmt(op, a, b, out, n, fmt_in, fmt_out, 0))
    out = bytes(out)
    return [out[_size(fmt_out) * i:_size(fmt_out) * (i + 1)] for i in range(n)]


def verdict(L, form, a, b, target, n, fmt_in):
    assert len(a) == n * _size(fmt_in) and len(target) == 384
    out = (C.c_uint8 * n)(*([0xEE] * n))
    _chk(L, L.bn254_dbg_verdict(form, a, b, target, out, n, fmt_in, 0))
    return list(bytes(out))


# ---------------------------------------------------------------------------------------------------------------- operands
def _r12(rng):
    return [rng.randrange(P) for _ in range(12)]


def _single(rng, k):
    """one non-zero Fp2 coefficient, at tower position k (0..5)"""
    v = [0] * 12
    v[2 * k], v[2 * k + 1] = rng.randrange(1, P), rng.randrange(1, P)
    return v


def edge_values(rng, with_zero):
    """13 different values: 1, -1, 0 (or a random value where 0 is outside the operation's domain), an element of Fp, of Fp2, c0 = 0, c1 = 0, and a single non-zero
    coefficient at each of the six positions"""
    v = [[1] + [0] * 11, [P - 1] + [0] * 11, [0] * 12 if with_zero else _r12(rng), [rng.randrange(2, P - 1)] + [0] * 11,
         [rng.randrange(1, P), rng.randrange(1, P)] + [0] * 10, [0] * 6 + _r12(rng)[:6], _r12(rng)[:6] + [0] * 6]
    v += [_single(rng, k) for k in range(6)]
    assert len(v) == NC and len({tuple(x) for x in v}) == NC
    return v


def _g1g2(O, rng):
    return O.g1_mul(O.g1_gen(), rng.randrange(1, R)), O.g2_mul(O.g2_gen(), rng.randrange(1, R))


@pytest.fixture(scope="module")
def operands(O):
    """The operand lists every test shares: computed once, never modified."""
    rng = random.Random(0xC12)
    edge = edge_values(rng, True)
    edge_inv = edge_values(rng, False)
    rand = [_r12(rng) for _ in range(NC - 2)] + [D.vals12(O.miller_loop(*_g1g2(O, rng))) for _ in range(2)]   # random values and Miller-loop outputs
    rand2 = [_r12(rng) for _ in range(NC)]
    cyc = []
    for _ in range(NC):                                                       # cyclotomic: the easy part of the final exponentiation of a random value
        x = D.bytes12(_r12(rng))
        c = O.fp12_op(O_MUL, O.fp12_op(O_CONJ, x), O.fp12_op(O_INV, x))
        cyc.append(D.vals12(O.fp12_op(O_MUL, O.fp12_op(O_FROB2, c), c)))
    lanes = (edge + rand + rand2 + cyc + [_r12(rng) for _ in range(NL_)])[:NL_]
    lanes_b = [_r12(rng) for _ in range(NL_ - NC)] + edge
    assert len({tuple(x) for x in lanes}) == NL_
    return {"edge": edge, "edge_inv": edge_inv, "rand": rand, "rand2": rand2, "cyc": cyc, "lanes": lanes, "lanes_b": lanes_b}


def _cat(vals):
    return b"".join(D.bytes12(v) for v in vals)


def _line(rng, fp2_d0):
    """a sparse line d0 + d3 w + d4 w^3 as the full Fp12 value: tower coefficient c0.c0 = d0, c1.c0 = d3, c1.c1 = d4"""
    v = [0] * 12
    v[0] = rng.randrange(1, P)
    if fp2_d0:
        v[1] = rng.randrange(1, P)
    v[6], v[7], v[8], v[9] = (rng.randrange(P) for _ in range(4))
    return v


def _expect1(O, oop, vals):
    return [O.fp12_op(oop, D.bytes12(v)) for v in vals]


def _expect2(O, a, b, conj_a=False, conj_b=False):
    out = []
    for x, y in zip(a, b):
        xb, yb = D.bytes12(x), D.bytes12(y)
        out.append(O.fp12_op(O_MUL, O.fp12_op(O_CONJ, xb) if conj_a else xb, O.fp12_op(O_CONJ, yb) if conj_b else yb))
    return out


def _sqr_n(O, v, count):
    x = D.bytes12(v)
    for _ in range(count):
        x = O.fp12_op(O_SQR, x)
    return x


# ---------------------------------------------------------------------------------------------------------------- operations against the oracle
@pytest.mark.parametrize("op,conj_a,conj_b", [(MUL, False, False), (MUL_CONJ_B, False, True), (MUL_CONJ_A, True, False)])
def test_coop12_products(L, O, operands, op, conj_a, conj_b):
    """c12_mul through Coop12Ops: plain, with conj_b, and with the first operand flagged VE_CONJ (rewritten as conj(a conj(b)))."""
    for a, b in ((operands["edge"], operands["rand"]), (operands["rand"], operands["edge"]), (operands["rand"], operands["rand2"]), (operands["edge"], operands["edge"])):
        got = coop_op(L, op, _cat(a), _cat(b), NC)
        assert got == _expect2(O, a, b, conj_a, conj_b), op


def test_coop12_unary_operations(L, O, operands):
    """c12_sqr, c12_conj, c12_frob (j = 1, 2, 3), c12_inv on edge operands, random values and Miller-loop outputs."""
    for name in ("edge", "rand"):
        vals = operands[name]
        a = _cat(vals)
        assert coop_op(L, SQR, a, None, NC) == _expect1(O, O_SQR, vals), name
        assert coop_op(L, CONJ, a, None, NC) == _expect1(O, O_CONJ, vals), name
        for j, oop in ((1, O_FROB1), (2, O_FROB2), (3, O_FROB3)):
            assert coop_op(L, FROB, a, None, NC, arg=j) == _expect1(O, oop, vals), (name, j)
    for name in ("edge_inv", "rand"):
        vals = operands[name]
        assert coop_op(L, INV, _cat(vals), None, NC) == _expect1(O, O_INV, vals), name


@pytest.mark.parametrize("count", [1, 2, LONGEST_RUN])
def test_coop12_cyclotomic_squarings(L, O, operands, count):
    """c12_cyclo_sqr_n on values of the cyclotomic subgroup against `count` general squarings of the oracle."""
    vals = operands["cyc"]
    assert coop_op(L, CYCLO_N, _cat(vals), None, NC, arg=count) == [_sqr_n(O, v, count) for v in vals]


def test_coop12_sparse_line_products(L, O, operands):
    """c12_mul_line_fp (keep off and on) and c12_mul_line_fp2 against the FULL oracle product with the line embedded at w^0, w^1, w^3."""
    rng = random.Random(0x11E)
    for name in ("edge", "rand"):
        a = operands[name]
        lf, lf2 = [_line(rng, False) for _ in range(NC)], [_line(rng, True) for _ in range(NC)]
        assert coop_op(L, LINE_FP, _cat(a), _cat(lf), NC) == _expect2(O, a, lf), name
        assert coop_op(L, LINE_FP_KEEP, _cat(a), _cat(lf), NC) == [D.bytes12(v) for v in a], name
        assert coop_op(L, LINE_FP2, _cat(a), _cat(lf2), NC) == _expect2(O, a, lf2), name


def test_lane_fp12_ops_on_edge_operands(L, O, operands):
    """The lane kernels behind bn254_dbg_fp12_op on the edge operands (they had only seen random ones), 70 proofs: two wavefronts."""
    a, b = operands["lanes"], operands["lanes_b"]
    ab, bb = _cat(a), _cat(b)
    assert lane_op(L, 0, ab, bb, NL_) == _expect2(O, a, b)
    assert lane_op(L, 8, ab, bb, NL_) == _expect2(O, a, b, conj_b=True)
    assert lane_op(L, 9, ab, bb, NL_) == _expect2(O, a, b, conj_a=True)
    assert lane_op(L, 1, ab, None, NL_) == _expect1(O, O_SQR, a)
    for op, oop in ((4, O_FROB1), (6, O_FROB2), (7, O_FROB3)):
        assert lane_op(L, op, ab, None, NL_) == _expect1(O, oop, a), op
    inv = [v if any(v) else [7] + [0] * 11 for v in a]                        # 0 has no inverse
    assert lane_op(L, 2, _cat(inv), None, NL_) == _expect1(O, O_INV, inv)
    cyc = (operands["cyc"] * 6)[:NL_]
    cyc = [D.vals12(_sqr_n(O, v, i // NC)) for i, v in enumerate(cyc)]        # 70 different cyclotomic values
    assert len({tuple(v) for v in cyc}) == NL_
    assert lane_op(L, 5, _cat(cyc), None, NL_) == [_sqr_n(O, v, 1) for v in cyc]


# ---------------------------------------------------------------------------------------------------------------- representatives
def _representatives(vals, seed):
    """The same field values as raw digits: number t of proof i as m, m + p or m - p in turn, m = x 2^261 mod p.  Every choice is inside the input contract
    (asserted, with Python integers, before anything reaches the GPU)."""
    out = []
    for i, v in enumerate(vals):
        reps = [D.encode(D.mont(x) + ((i + t + seed) % 3 - 1) * P) for t, x in enumerate(v)]
        assert all(D.in_contract(d) for d in reps) and [D.field_value(d) for d in reps] == [x % P for x in v]
        out.append(reps)
    return out


def _pattern_values(n, seed):
    """n Fp12 values whose twelve residues are picked for their digits: the eight low digits all -2^28, all 2^28 - 1, or alternating, under a small top digit"""
    out = []
    for i in range(n):
        reps = [D.pattern((i + t) % 4, 1 + seed + 12 * i + t) for t in range(12)]
        assert all(D.in_contract(d) for d in reps)
        out.append(reps)
    vals = [[D.field_value(d) for d in reps] for reps in out]
    assert len({tuple(v) for v in vals}) == n
    return out, vals


def _pack(reps):
    return b"".join(D.pack12(r) for r in reps)


def _decoded(got):
    """raw-digit results -> the 384 bytes of their field values.  What a kernel stores is itself a legal operand of the next one: |digit| <= 2^28 (a negation turns
    -2^28 into 2^28) and |value| < 3 p (the sum of two reduced dot products, the widest value an operation emits, is below 2.42 p)"""
    out = []
    for g in got:
        ds = D.unpack12(g)
        assert all(D.in_contract(d, 3, negated=True) for d in ds)
        out.append(D.bytes12([D.field_value(d) for d in ds]))
    return out


def _representative_sets(operands, n, key_a, key_b):
    ra, rb = _representatives(operands[key_a][:n], 0), _representatives(operands[key_b][:n], 1)
    pa, va = _pattern_values(n, 0)
    pb, vb = _pattern_values(n, 1000)
    return ((ra, operands[key_a][:n], rb, operands[key_b][:n]), (pa, va, pb, vb), (pa, va, rb, operands[key_b][:n]))


def test_coop12_operations_on_chosen_representatives(L, O, operands):
    """Every cooperative operation on raw-digit operands: m, m + p, m - p of the same values, and residues with extreme digit patterns (the column accumulators'
    worst case).  The result, decoded to a field value, must be the integer result."""
    rng = random.Random(0x5EED)
    for ra, va, rb, vb in _representative_sets(operands, NC, "rand", "rand2"):
        a, b = _pack(ra), _pack(rb)
        for op, ca, cb in ((MUL, False, False), (MUL_CONJ_B, False, True), (MUL_CONJ_A, True, False)):
            assert _decoded(coop_op(L, op, a, b, NC, 1, 1)) == _expect2(O, va, vb, ca, cb), op
        assert _decoded(coop_op(L, SQR, a, None, NC, 1, 1)) == _expect1(O, O_SQR, va)
        assert _decoded(coop_op(L, CONJ, a, None, NC, 1, 1)) == _expect1(O, O_CONJ, va)
        assert _decoded(coop_op(L, INV, a, None, NC, 1, 1)) == _expect1(O, O_INV, va)
        for j, oop in ((1, O_FROB1), (2, O_FROB2), (3, O_FROB3)):
            assert _decoded(coop_op(L, FROB, a, None, NC, 1, 1, arg=j)) == _expect1(O, oop, va), j
        # the line's own numbers as representatives too: zero coefficients stay the digits of 0, +p or -p
        lf, lf2 = [_line(rng, False) for _ in range(NC)], [_line(rng, True) for _ in range(NC)]
        assert _decoded(coop_op(L, LINE_FP, a, _pack(_representatives(lf, 2)), NC, 1, 1)) == _expect2(O, va, lf)
        assert _decoded(coop_op(L, LINE_FP_KEEP, a, _pack(_representatives(lf, 2)), NC, 1, 1)) == [D.bytes12(v) for v in va]
        assert _decoded(coop_op(L, LINE_FP2, a, _pack(_representatives(lf2, 0)), NC, 1, 1)) == _expect2(O, va, lf2)
        # the final exponentiation, raw digits in, bytes out
        assert coop_op(L, FINAL_EXP, a, None, NC, 1, 0) == [O.final_exp(D.bytes12(v)) for v in va]
    cyc = operands["cyc"]
    for count in (1, LONGEST_RUN):
        assert _decoded(coop_op(L, CYCLO_N, _pack(_representatives(cyc, count)), None, NC, 1, 1, arg=count)) == [_sqr_n(O, v, count) for v in cyc], count


def test_lane_operations_on_chosen_representatives(L, O, operands):
    """The same through the lane kernels, 70 proofs."""
    for ra, va, rb, vb in _representative_sets(operands, NL_, "lanes", "lanes_b"):
        a, b = _pack(ra), _pack(rb)
        for op, ca, cb in ((0, False, False), (8, False, True), (9, True, False)):
            assert _decoded(lane_op(L, op, a, b, NL_, 1, 1)) == _expect2(O, va, vb, ca, cb), op
        assert _decoded(lane_op(L, 1, a, None, NL_, 1, 1)) == _expect1(O, O_SQR, va)
        for op, oop in ((4, O_FROB1), (6, O_FROB2), (7, O_FROB3)):
            assert _decoded(lane_op(L, op, a, None, NL_, 1, 1)) == _expect1(O, oop, va), op
        inv = [(r, v) if any(v) else (r[:0] + [D.encode(D.mont(7))] + r[1:], [7] + v[1:]) for r, v in zip(ra, va)]
        assert _decoded(lane_op(L, 2, _pack([r for r, _ in inv]), None, NL_, 1, 1)) == _expect1(O, O_INV, [v for _, v in inv])
    cyc = [D.vals12(_sqr_n(O, v, i // NC)) for i, v in enumerate((operands["cyc"] * 6)[:NL_])]
    assert _decoded(lane_op(L, 5, _pack(_representatives(cyc, 0)), None, NL_, 1, 1)) == [_sqr_n(O, v, 1) for v in cyc]


# ---------------------------------------------------------------------------------------------------------------- final exponentiation
def test_coop12_final_exp_edge_values(L, O):
    """k_coop12_final_exp on the edge list of the host test (test_final_exp_program_without_conjugations): random values, 1, -1, an element of Fp, c1 = 0, c0 = 0,
    an element of Fp2, 3 v, Miller-loop outputs and values already in the cyclotomic subgroup."""
    rng = random.Random(0xF07D)
    r12 = lambda: D.bytes12(_r12(rng))
    one = be(1) + bytes(352)
    cases = [r12(), r12(), one, be(P - 1) + bytes(352), be(rng.randrange(1, P)) + bytes(352), r12()[:192] + bytes(192), bytes(192) + r12()[:192],
             be(rng.randrange(P)) + be(rng.randrange(P)) + bytes(320), bytes(64) + be(3) + bytes(288)]
    for _ in range(2):
        pa, qb = _g1g2(O, rng)
        cases += [O.miller_loop(pa, qb), O.pairing(pa, qb)]
    assert len(cases) == NC and len(set(cases)) == NC
    assert coop_op(L, FINAL_EXP, b"".join(cases), None, NC) == [O.final_exp(f) for f in cases]


# ---------------------------------------------------------------------------------------------------------------- near-miss compares
def _verdict_cases(target_vals):
    """(digits of twelve numbers, expected verdict) around a target: the exact value in canonical digits; each single number as t + p and as t - p (a zero of the
    target thus as p and as -p); several numbers moved at once; and exactly one number off by one unit of its residue, in canonical digits and on top of + p and - p."""
    m = [D.mont(t) for t in target_vals]
    canon = [D.encode(x) for x in m]
    cases = [(canon, ACCEPT)]
    for t in range(12):
        for s in (1, -1):
            cases.append((canon[:t] + [D.encode(m[t] + s * P)] + canon[t + 1:], ACCEPT))
    for k in range(3):
        cases.append(([D.encode(m[t] + ((t + k) % 3 - 1) * P) for t in range(12)], ACCEPT))
    for t in range(12):
        for off in (1, -1):
            for s in (0, 1, -1):
                cases.append((canon[:t] + [D.encode(m[t] + off + s * P)] + canon[t + 1:], REJECT))
    for reps, _ in cases:
        assert all(D.in_contract(d) for d in reps)                            # |m + 1 + p| < 2 p and |m - 1 - p| <= p + 1
    return cases


def _targets():
    rng = random.Random(0x7A6)
    return [_r12(rng), [1] + [0] * 11]


@pytest.mark.parametrize("form,n", [(0, NL_), (2, NC)])
def test_compare_near_misses(L, form, n):
    """k_g16_compare (form 0) and c12_eq_const (form 2) against a random target and against 1 (PlonK's: eleven zeros, each of which may arrive as 0, p or -p): the
    target in any representative ACCEPTS, one number of twelve off by one REJECTS -- 24 cases per target, also on top of a + p or - p representative."""
    for tv in _targets():
        cases = _verdict_cases(tv)
        assert sum(1 for _, e in cases if e == REJECT) == 72
        for lo in range(0, len(cases), n):
            chunk = cases[lo:lo + n]
            chunk = chunk + cases[:n - len(chunk)]
            got = verdict(L, form, _pack([r for r, _ in chunk]), None, D.bytes12(tv), n, 1)
            assert got == [e for _, e in chunk], (form, lo)
        # canonical bytes: the loader's conversion of the operand
        got = verdict(L, form, D.bytes12(tv) * n, None, D.bytes12(tv), n, 0)
        assert got == [ACCEPT] * n


def test_coop12_compare_votes_per_proof_position(L):
    """c12_eq_const votes per proof with (ballot >> 12 pl) & 0xfff: ONE bad proof (a single number off by one) at every position of the batch -- wavefront positions
    pl = 0 .. 4, and the last proof of the partly filled third wavefront -- among exact matches in differing representatives: exactly that proof rejects.  The bad
    number walks over the twelve lanes of the group."""
    for tv in _targets():
        m = [D.mont(t) for t in tv]
        for pos in range(NC):
            vals = [[D.encode(m[t] + ((i + t) % 3 - 1) * P) for t in range(12)] for i in range(NC)]
            t_bad = (pos * 5 + 3) % 12
            vals[pos][t_bad] = D.encode(m[t_bad] + (1 if pos % 2 else -1))
            assert all(D.in_contract(d) for reps in vals for d in reps)
            got = verdict(L, 2, _pack(vals), None, D.bytes12(tv), NC, 1)
            assert got == [REJECT if i == pos else ACCEPT for i in range(NC)], (pos, t_bad)


def test_mul_verdict_near_misses(L, O):
    """k_f12_mul_verdict compares a b as it stores it: a random and invertible, b = a^-1 t' from the oracle.  t' = the target ACCEPTS; t' = the target with exactly one
    of its twelve numbers off by +-1 REJECTS (24 cases per target); the operands as bytes and as m, m + p, m - p digits."""
    rng = random.Random(0x3E1)
    for tv in _targets():
        want, a_vals, b_vals = [], [], []
        for i in range(NL_):
            tp = list(tv)
            if i % 2 == 1 and i // 2 < 24:
                k = i // 2
                tp[k // 2] = (tp[k // 2] + (1 if k % 2 else -1)) % P
            a = _r12(rng)
            b = D.vals12(O.fp12_op(O_MUL, O.fp12_op(O_INV, D.bytes12(a)), D.bytes12(tp)))
            assert O.fp12_op(O_MUL, D.bytes12(a), D.bytes12(b)) == D.bytes12(tp)
            a_vals.append(a); b_vals.append(b); want.append(ACCEPT if tp == list(tv) else REJECT)
        assert want.count(REJECT) == 24
        assert verdict(L, 1, _cat(a_vals), _cat(b_vals), D.bytes12(tv), NL_, 0) == want
        assert verdict(L, 1, _pack(_representatives(a_vals, 0)), _pack(_representatives(b_vals, 1)), D.bytes12(tv), NL_, 1) == want


# ---------------------------------------------------------------------------------------------------------------- whole kernels
def _g2_neg(q):
    return q[:64] + be((P - int.from_bytes(q[64:96], "big")) % P) + be((P - int.from_bytes(q[96:128], "big")) % P)


@pytest.fixture(scope="module")
def key(pkg, O):
    """A synthetic gnark key prepared in gnark mode, and its points from the oracle's decoders.  bn254_host.hpp::prepare_g16, mode 1: table 0 holds the lines of
    -gamma, table 1 those of -delta, the target is e(alpha, beta)."""
    vk, proofs, inputs, expected = pkg.synth_groth16(0xC0012, 2, NC, invalid_every=2, agree=True, threads=4, l_identity=True)
    dec2 = lambda b: O.decompress_g2(b, O.MODE_GNARK)
    (s1, alpha), (s2, beta), (s3, gamma), (s4, delta) = O.decompress_g1(vk[0:32]), dec2(vk[64:128]), dec2(vk[128:192]), dec2(vk[224:288])
    ks = [O.decompress_g1(vk[292 + 32 * i:324 + 32 * i]) for i in range(3)]
    assert {s1, s2, s3, s4} | {s for s, _ in ks} == {O.ACCEPT}
    pvk = pkg.PreparedVk(vk, pkg.VK_GNARK)
    yield {"pvk": pvk, "neg_gamma": _g2_neg(gamma), "neg_delta": _g2_neg(delta), "target": O.pairing(alpha, beta), "k": [k for _, k in ks],
           "proofs": proofs, "inputs": inputs, "expected": expected}
    pvk.close()


def _gt_product(O, pairs):
    """prod e(P, Q) over the pairs whose G1 point is not the identity"""
    pairs = [(p, q) for p, q in pairs if p is not None]
    if not pairs:
        return be(1) + bytes(352)
    return O.pairing(b"".join(p for p, _ in pairs), b"".join(q for _, q in pairs))


def test_coop12_miller_fixed_values(L, O, key):
    """k_coop12_miller_fixed in its store mode (target == nullptr) with the key's tables: the GT value is e(P0, -gamma) [e(P1, -delta)] -- a key prepared in gnark
    mode holds the lines of the NEGATED gamma and delta (bn254_host.hpp::prepare_g16) -- for one and two pairs, with the identity flag on each pair in turn (its
    factor is then 1 whatever bytes the point holds)."""
    rng = random.Random(0xF1D)
    p0 = [O.g1_mul(O.g1_gen(), rng.randrange(1, R)) for _ in range(NC)]
    p1 = [O.g1_mul(O.g1_gen(), rng.randrange(1, R)) for _ in range(NC)]
    for n_pairs in (1, 2):
        for flags in ([0] * NC, [(i % 3) if n_pairs == 2 else (i % 2) for i in range(NC)], [3 if n_pairs == 2 else 1] * NC):
            out = (C.c_uint8 * (384 * NC))()
            _chk(L, L.bn254_dbg_coop12_miller_fixed(key["pvk"].handle, n_pairs, b"".join(p0), b"".join(p1) if n_pairs == 2 else None, bytes(flags), out, NC, 0))
            out = bytes(out)
            for i in range(NC):
                pairs = [(None if flags[i] & 1 else p0[i], key["neg_gamma"])]
                if n_pairs == 2:
                    pairs.append((None if flags[i] & 2 else p1[i], key["neg_delta"]))
                assert out[384 * i:384 * i + 384] == _gt_product(O, pairs), (n_pairs, flags[i], i)


def test_coop12_miller_g16_values(L, O, key):
    """k_coop12_miller_g16 in its store mode (no target) on a 13-proof synthetic batch: every failure class (wrong input, wrong C, B outside G2 reach the pairing;
    A off the curve and A.x >= p stop at the loader) and proofs whose public-input point L is the identity.  The GT value of every proof that reaches the pairing is
    e(A, B) e(L, -gamma) e(C, -delta) of the oracle, with L from the oracle's group law; for an accepted proof it is also the key's target e(alpha, beta)."""
    out, st = (C.c_uint8 * (384 * NC))(), (C.c_uint8 * NC)()
    _chk(L, L.bn254_dbg_coop12_miller_g16(key["pvk"].handle, key["proofs"], key["inputs"], 2, NC, out, st, 0))
    out, st, exp = bytes(out), list(bytes(st)), list(key["expected"])
    assert set(exp) == {O.REJECT, O.ACCEPT, O.ERR_NOT_MEMBER, O.ERR_NOT_ON_CURVE, O.ERR_NOT_IN_SUBGROUP}
    seen_linf = 0
    for i in range(NC):
        reached = exp[i] in (O.ACCEPT, O.REJECT, O.ERR_NOT_IN_SUBGROUP)
        assert (st[i] == O.ACCEPT) == reached, (i, st[i], exp[i])
        if not reached:
            assert st[i] == exp[i], i
            continue
        pr = key["proofs"][256 * i:256 * i + 256]
        xs = [int.from_bytes(key["inputs"][64 * i + 32 * s:64 * i + 32 * s + 32], "big") for s in range(2)]
        # L = K0 + x0 K1 + x1 K2 (scalars as raw integers): all-zero bytes from the oracle's group law are the identity
        acc = key["k"][0]
        for s in range(2):
            t = O.g1_mul(key["k"][s + 1], xs[s] % R)
            acc = t if acc == bytes(64) else acc if t == bytes(64) else O.g1_add(acc, t)
        l_pt = None if acc == bytes(64) else acc
        seen_linf += l_pt is None
        want = _gt_product(O, [(pr[0:64], pr[64:192]), (l_pt, key["neg_gamma"]), (pr[192:256], key["neg_delta"])])
        assert out[384 * i:384 * i + 384] == want, (i, exp[i])
        assert (want == key["target"]) == (exp[i] == O.ACCEPT), i
    assert seen_linf >= 1
