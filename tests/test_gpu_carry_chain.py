"""GPU tests of the carry-first multiply-add chains of csrc/bn254_fp.h / bn254_tower.h (BN_OPQ, the explicit squares psq / DotSq): the lane kernels through the existing
probes at 64 lanes (one full wavefront) and 257 (a partial wavefront past a 256-thread workgroup), on the operands where a mis-ordered carry or a wrong doubled
cross term shows -- digits at -2^28, 2^28 - 1 and +2^28 in every column, and the loosest representatives the input contract admits (m + p, m - p: tests/fp12_digits.py).
Bit for bit against the CPU oracle and Python integers; one Groth16 batch of 257 proofs with all five failure classes against the generator."""
import ctypes as C
import random

import pytest

import fp12_digits as D

pytestmark = pytest.mark.gpu
P = D.P
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SIZES = (64, 257)
NMAX = max(SIZES)
O_MUL, O_SQR, O_INV, O_FROB1, O_FROB2, O_FROB3, O_CYCLO, O_CONJ = range(8)


def be(v):
    return int(v).to_bytes(32, "big")


@pytest.fixture(scope="module")
def L(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    lib = pkg.lib()
    lib.bn254_dbg_fp12_op_fmt.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int]
    return lib


def lane_op(L, op, a, b, n):
    """bn254_dbg_fp12_op_fmt: operands as raw digits (format 1), the result as canonical bytes (format 0)"""
    assert len(a) == 432 * n and (b is None or len(b) == 432 * n)
    out = (C.c_uint8 * (384 * n))()
    assert L.bn254_dbg_fp12_op_fmt(op, a, b, out, n, 1, 0, 0) == 0, L.bn254_last_error()
    out = bytes(out)
    return [out[384 * i:384 * (i + 1)] for i in range(n)]


def _digit_operands(n, seed, rng, negated):
    """n Fp12 operands as digit lists, every one different.  Proof i, number t: a pattern residue (eight low digits all -2^28, all 2^28 - 1 or alternating) for
    i % 3 == 0 -- negated digit-wise (digits +2^28 and -(2^28 - 1)) where `negated` -- and otherwise a random residue m as m + p or m - p (|value| up to 2 p)."""
    out = []
    for i in range(n):
        reps = []
        for t in range(12):
            if i % 3 == 0:
                d = D.pattern((i // 3 + t) % 4, 1 + seed + 12 * i + t)
                if negated and (i // 3) % 2:
                    d = [-x for x in d]
            else:
                d = D.encode(D.mont(rng.randrange(P)) + (P if (i + t) % 2 else -P))
            assert D.in_contract(d, negated=negated)
            reps.append(d)
        out.append(reps)
    assert len({tuple(map(tuple, r)) for r in out}) == n
    return out


def _vals(reps):
    return [[D.field_value(d) for d in r] for r in reps]


def _pack(reps):
    return b"".join(D.pack12(r) for r in reps)


@pytest.fixture(scope="module")
def operands(O):
    """Computed once for both sizes (the 64-lane runs take the first 64), never modified."""
    rng = random.Random(0xCA44)
    a = _digit_operands(NMAX, 0, rng, True)
    b = _digit_operands(NMAX, 5000, rng, False)
    b = b[1:] + b[:1]                                              # pattern x loose, loose x pattern and, every third pair apart, pattern x pattern
    b[0::9] = _digit_operands(NMAX, 9000, rng, True)[0::9]
    va, vb = _vals(a), _vals(b)
    ab, bb = [D.bytes12(v) for v in va], [D.bytes12(v) for v in vb]
    # cyclotomic values (the easy part of the final exponentiation of the a's), as loose representatives m + p / m - p
    cyc_v = []
    for x in ab[:NMAX]:
        c = O.fp12_op(O_MUL, O.fp12_op(O_CONJ, x), O.fp12_op(O_INV, x))
        cyc_v.append(D.vals12(O.fp12_op(O_MUL, O.fp12_op(O_FROB2, c), c)))
    cyc = [[D.encode(D.mont(x) + (P if (i + t) % 2 else -P)) for t, x in enumerate(v)] for i, v in enumerate(cyc_v)]
    assert all(D.in_contract(d) for r in cyc for d in r) and _vals(cyc) == cyc_v
    return {"a": a, "b": b, "cyc": cyc,
            "mul": [O.fp12_op(O_MUL, x, y) for x, y in zip(ab, bb)], "sqr": [O.fp12_op(O_SQR, x) for x in ab],
            "mul_cb": [O.fp12_op(O_MUL, x, O.fp12_op(O_CONJ, y)) for x, y in zip(ab, bb)],
            "inv": [O.fp12_op(O_INV, x) for x in ab], "cyc_sqr": [O.fp12_op(O_SQR, D.bytes12(v)) for v in cyc_v]}


@pytest.mark.parametrize("n", SIZES)
def test_fp_mul_probe(L, n):
    """k_dbg_fp_mul (fp_dot with one term, the two conversions' fp_mul and fp_reduce): values whose low digits are all-ones / all-zero patterns, and random ones."""
    rng = random.Random(0xCA01 + n)
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 253, (1 << 254) - 1, (1 << 256) - 1, 3, 9, D.R261_INV, P - D.R261_INV]
    edge += [(1 << (29 * k)) - 1 for k in range(1, 9)] + [1 << (29 * k - 1) for k in range(1, 9)] + [P - (1 << (29 * k - 1)) for k in range(1, 9)]
    # residues picked for their Montgomery digits: x with x 2^261 = a digit pattern
    edge += [D.field_value(D.pattern(k, top)) for k in range(4) for top in (1, 7)]
    xs = (edge + [rng.randrange(P) for _ in range(n)])[:n]
    ys = (list(reversed(edge)) + [rng.randrange(P) for _ in range(n)])[:n]
    out = (C.c_uint8 * (32 * n))()
    assert L.bn254_dbg_fp_mul(b"".join(map(be, xs)), b"".join(map(be, ys)), out, C.c_size_t(n), 0) == 0, L.bn254_last_error()
    out = bytes(out)
    assert [int.from_bytes(out[32 * i:32 * i + 32], "big") for i in range(n)] == [x * y % P for x, y in zip(xs, ys)]


@pytest.mark.parametrize("n", SIZES)
def test_fp12_lane_ops_on_extreme_digits(L, operands, n):
    """k_f12_mul (fp2_dotk), the fused conjugation, k_f12_sqr (fp2_dotp with psq terms), k_f12_inv (fp6_sqr, fp6_inv: psq, dsq) and k_f12_cyclo_sqr (the form that
    keeps the reassociated chains) on raw-digit operands."""
    a, b = _pack(operands["a"][:n]), _pack(operands["b"][:n])
    assert lane_op(L, 0, a, b, n) == operands["mul"][:n]
    assert lane_op(L, 8, a, b, n) == operands["mul_cb"][:n]
    assert lane_op(L, 1, a, None, n) == operands["sqr"][:n]
    assert lane_op(L, 2, a, None, n) == operands["inv"][:n]
    assert lane_op(L, 5, _pack(operands["cyc"][:n]), None, n) == operands["cyc_sqr"][:n]


@pytest.mark.parametrize("n", SIZES)
def test_pairing_probe(L, O, n):
    """bn254_dbg_pairing: k_miller_run (both forms of line, the G2 steps), the final exponentiation's products, squarings and Frobenius maps.  Sixteen different pairs,
    laid out so that neighbouring lanes differ; the oracle computes each once."""
    rng = random.Random(0xCA02)
    g1, g2 = O.g1_gen(), O.g2_gen()
    ps = [O.g1_mul(g1, k) for k in [1, R - 1, 2] + [rng.randrange(1, R) for _ in range(13)]]
    qs = [O.g2_mul(g2, k) for k in [1, 2, R - 1] + [rng.randrange(1, R) for _ in range(13)]]
    want = [O.pairing(p, q) for p, q in zip(ps, qs)]
    idx = [(7 * i + i // 16) % 16 for i in range(n)]
    out = (C.c_uint8 * (384 * n))()
    assert L.bn254_dbg_pairing(b"".join(ps[j] for j in idx), b"".join(qs[j] for j in idx), out, C.c_size_t(n), 0) == 0, L.bn254_last_error()
    out = bytes(out)
    assert [out[384 * i:384 * i + 384] for i in range(n)] == [want[j] for j in idx]


def test_groth16_batch_257_all_failure_classes(pkg, O, L):
    """257 proofs, every fourth invalid, the five failure classes in turn: the status bytes of the generator, and the oracle's on a prefix that holds every class."""
    n = 257
    vk, proofs, inputs, exp = pkg.synth_groth16(0xB254CA44, 2, n, invalid_every=4, agree=True, threads=8)
    assert set(exp) == {0, 1, 2, 3, 4}
    pvk = pkg.PreparedVk(vk)
    st = pvk.verify_batch(proofs, inputs)
    assert st == exp
    m = 24
    assert set(exp[:m]) == {0, 1, 2, 3, 4} and O.groth16_verify_many(proofs[:256 * m], 256, vk, inputs[:64 * m], 2, m, O.MODE_REFERENCE) == st[:m]
    pvk.close()
