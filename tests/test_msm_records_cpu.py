"""The CPU half of tests/test_gpu_g1_msm_values.py: every case of its first group, as tests/msm_records.py builds it, goes item by item through the rows of
csrc/bn254_msm.h compiled for the host (tests/hostsim's hs_msm_rows_joint, bound tracker on) and must give the oracle's sums -- so the inputs and the expectations are
known to be right before a GPU sees them, and a GPU failure of the same case is a device-only fault.  Plus: the table of small multiples against O.g1_mul, the
representatives of the row-sum tests under the tracker, and the refusals of the three probes (no device is reached: validation comes first)."""
import ctypes as C
import random
import struct

import pytest

import fp12_digits as D
import msm_records as M

NO_DEVICE = 1 << 20          # an ordinal no machine has
E_BAD_ARG = -1
REFUSED, PAST = "refused by the checks", "got as far as the device"


def _verdict(L, rc):
    """what became of a probe call with device = NO_DEVICE: refused by the argument checks, or past them -- then the device lookup fails, with BN254_E_NO_DEVICE on
    a machine without a GPU and with BN254_E_BAD_ARG "device ordinal out of range" on one with GPUs"""
    assert rc != 0, "no device has this ordinal"
    err = L.bn254_last_error()
    err = err.decode() if isinstance(err, bytes) else str(err)
    return REFUSED if rc == E_BAD_ARG and "device ordinal" not in err else PAST


@pytest.mark.parametrize("name", M.case_names())
def test_case_on_the_host_rows(hostsim, pkg, O, name):
    c = M.build_case(pkg.lib(), O, name)
    n_pad = (c["n"] + 63) // 64 * 64
    if c["granule_key"]:
        got, info = [], None
        for i in range(c["n"]):
            nt = c["n_terms"]
            g, info = M.host_sums(hostsim, c["sums"], nt, c["records"][129 * nt * i:129 * nt * (i + 1)], M.item_bases(c, i), 1, n_pad, c["budget"], c["joint_g"])
            got += g
    else:
        got, info = M.host_sums(hostsim, c["sums"], c["n_terms"], c["records"], c["bases"], c["n"], n_pad, c["budget"], c["joint_g"])
    bad = [(i, s) for i in range(c["n"]) for s in range(len(c["sums"])) if got[i][s] != c["want"][i][s]]
    assert not bad, (name, bad[:8])
    assert info[0] <= M.MAX_ROWS


def test_point_cases_reach_the_identity(pkg, O):
    """the arrangement the workspace test relies on: items 8 .. 11 fill one status word with pending bytes whose sums are the identity, item 10 in both sums"""
    c = M.build_case(pkg.lib(), O, "points-split")
    st = M.status_in(c["n"])
    assert all(st[i] & M.PENDING for i in (8, 9, 10, 11))
    assert [[w == M.ID for w in c["want"][i]] for i in (8, 9, 10, 11)] == [[True, False], [False, True], [True, True], [True, False]]
    kinds = {M.point_kind(i) for i in range(c["n"])}
    assert kinds == set(M.POINT_KINDS)
    # identity sums under bytes that are NOT pending too: those bytes must stay as they are
    assert any(c["want"][i][0] == M.ID and not st[i] & M.PENDING for i in range(c["n"]))
    assert any(c["want"][i][1] == M.ID and not st[i] & M.PENDING for i in range(c["n"]))


def test_lambda_and_the_chosen_halves(pkg, O):
    lam, beta = M.lam_beta(O)
    g = O.g1_gen()
    assert O.g1_mul(g, lam) == M.be(beta * int.from_bytes(g[:32], "big") % M.P) + g[32:]
    L = pkg.lib()
    for k in (1, M.R - 1, lam, lam * lam % M.R, 12345, random.Random(5).randrange(M.R)):
        k1, k2, fl = M.glv(L, k)
        assert M.halves_scalar(O, int.from_bytes(k1, "big"), int.from_bytes(k2, "big"), fl & 2, fl & 4) == k % M.R
    # (lambda and lambda^2 need not come back as the halves (0, 1) and (1, 1): the rounding of the decomposition decides.  The cases write those halves themselves.)
    specs = M.var_scalar_specs(O)
    assert ("halves", (0, 1, 0, 0)) in specs and ("halves", (1, 0, 0, 0)) in specs and ("halves", (1, 1, 1, 1)) in specs
    assert M.halves_scalar(O, 0, 1, 0, 0) == lam and M.halves_scalar(O, 1, 1, 1, 1) == lam * lam % M.R


def test_fixed_scalars_cover_every_window():
    fs = M.fixed_scalar_specs()
    assert all(0 <= k < M.R for k in fs)
    digits = lambda k: [(k >> (M.FW_BITS * w)) & 8191 for w in range(M.FW_WINDOWS)]
    assert digits((1 << 247) - 1) == [8191] * 19 + [0]
    for w in range(M.FW_WINDOWS):
        assert any(d[w] and not any(d[:w] + d[w + 1:]) for d in map(digits, fs)), w       # a scalar whose only non-zero digit is digit w
    assert digits(M.R - 1)[M.FW_WINDOWS - 1] == (M.R - 1) >> 247


@pytest.fixture(scope="module")
def multiples(O):
    return M.Multiples(O)


def test_multiples_table(O, multiples):
    g = O.g1_gen()
    rng = random.Random(77)
    for m in [1, 2, 3, 63, 64, 65, 4095, 4096] + [rng.randrange(1, 4097) for _ in range(24)]:
        assert multiples(m) == O.g1_mul(g, m), m
        assert multiples(-m) == O.g1_mul(g, M.R - m), m
    assert multiples(0) == M.ID


def _sum_raw(hostsim, rows, lpi):
    out = (C.c_uint8 * 64)()
    hostsim.hs_g1_sum_rows_raw.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    assert hostsim.hs_g1_sum_rows_raw(out, b"".join(rows), len(rows), lpi) == 1
    return bytes(out)


def test_row_representatives_under_the_tracker(hostsim, O, multiples):
    """g1_add chains on rows declared at the bound k_g1_sum_affine declares when it loads one (|value| <= 3 p, low digits within 2^28), from the representatives the
    GPU test sends in format 1: every coordinate as m, m +- p, m +- 2 p, the extremes inside +-3 p, the digit patterns -- the bound tracker checks every
    operation of the additions, the oracle's table the sums."""
    rng = random.Random(78)
    for lpi, count in ((1, 3), (4, 4), (4, 5), (4, 14), (1, 14)):
        for trial in range(6):
            ms = [rng.randrange(-290, 291) or 1 for _ in range(count)]
            rows = []
            for j, m in enumerate(ms):
                x, y = multiples.xy(m)
                z = rng.randrange(2, M.P)
                co = [x * z % M.P, y * z % M.P, z]
                if trial < 5:
                    rows.append(M.raw_row([M.rep_digits(v, (trial + j + c) % 5 - 2) for c, v in enumerate(co)]))
                else:
                    rows.append(M.raw_row([M.extreme_rep(v, (j + c) & 1) for c, v in enumerate(co)]))
            assert _sum_raw(hostsim, rows, lpi) == multiples(sum(ms)), (lpi, count, trial)
    for kind in range(4):
        d, x, y = M.pattern_point(kind, rng)
        assert D.in_contract(d, 3)
        pt = M.be(x) + M.be(y)
        rows = [M.raw_row([d, M.rep_digits(y, 2), M.rep_digits(1, -2)]), M.raw_row([d, M.extreme_rep(y, True), M.extreme_rep(1, False)]), M.raw_row([d, M.rep_digits(y, 0), M.rep_digits(1, 0)])]
        assert _sum_raw(hostsim, rows[:1], 1) == pt
        assert _sum_raw(hostsim, rows, 1) == O.g1_mul(pt, 3)
        assert _sum_raw(hostsim, rows + rows[:1], 4) == O.g1_mul(pt, 4)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _msm_args(L):
    L.bn254_dbg_g1_msm.argtypes = [C.POINTER(C.c_int), C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint), C.c_size_t, C.c_size_t,
                                   C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]
    L.bn254_dbg_g1_sum_rows.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.bn254_dbg_plonk_group_sums.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_uint), C.c_int]


def test_probes_refuse_bad_arguments_before_any_device(pkg, O):
    """Each refusal is BN254_E_BAD_ARG although `device` names no device: the checks come first, and nothing is launched on what they refuse.  The same calls
    with good arguments get past them (and then fail on the device ordinal): the refusals are not an accident of something else."""
    L = pkg.lib()
    _msm_args(L)
    rng = random.Random(79)
    sums, nt = M.S1, M.T1
    n = 70
    records, bases, _ = M.build_items(L, O, rng, sums, nt, n)
    bb = b"".join(bases)
    out, inf, st, info = (C.c_uint8 * (128 * 256))(), (C.c_uint8 * 512)(), (C.c_uint8 * 256)(), (C.c_int * 6)()

    def msm(shape, n_terms=nt, n_bases=len(bases), n_keys=1, gk=None, items=n, budget=65536, joint_g=0, mode=0):
        sh = (C.c_int * len(shape))(*shape)
        g = (C.c_uint * len(gk))(*gk) if gk else None
        return _verdict(L, L.bn254_dbg_g1_msm(sh, len(shape), records, n_terms, bb * n_keys, n_bases, n_keys, g, items, budget, joint_g, mode, out, inf, st, info, NO_DEVICE))

    good = M.shape_list(sums)
    assert msm(good) == PAST
    assert list(info)[:5] == [11, 10, 11, 0, M.SPLIT]                    # the plan is made before the device is looked at
    assert msm(good, n_keys=2, gk=[1, 0]) == PAST
    bad_term = list(good); bad_term[4] = nt                             # the first variable term: one past the records
    bad_tab = list(good); bad_tab[-1] = len(bases)                      # the last table index: one past the bases
    neg_term = list(good); neg_term[4] = -1
    for what, rc in (("term index", msm(bad_term)), ("negative term index", msm(neg_term)), ("table index", msm(bad_tab)), ("key index", msm(good, n_keys=2, gk=[0, 2])),
                     ("no key indices", msm(good, n_keys=2)), ("n = 0", msm(good, items=0)), ("n above the cap", msm(good, items=32769)),
                     ("shape length", msm(good + [0])), ("three sums", msm([3] + good[1:])), ("n_terms = 0", msm(good, n_terms=0)),
                     ("too many rows", msm(M.shape_list([(list(range(16)), [], []), (list(range(16, 32)), [], [])]), n_terms=32, budget=64)),
                     ("too many variable terms", msm([1, 17, 0, 0] + list(range(17)), n_terms=17)), ("budget", msm(good, budget=63)), ("joint_g", msm(good, joint_g=9)),
                     ("mode", msm(good, mode=2))):
        assert rc == REFUSED, what
    off_curve = bb[:63] + bytes([bb[63] ^ 1]) + bb[64:]
    sh = (C.c_int * len(good))(*good)
    assert _verdict(L, L.bn254_dbg_g1_msm(sh, len(good), records, nt, off_curve, len(bases), 1, None, n, 65536, 0, 0, out, inf, st, info, NO_DEVICE)) == REFUSED
    big_x = b"\xff" * 32 + records[32:]                                 # the x of item 0's first point: not below p
    assert _verdict(L, L.bn254_dbg_g1_msm(sh, len(good), big_x, nt, bb, len(bases), 1, None, n, 65536, 0, 0, out, inf, st, info, NO_DEVICE)) == REFUSED
    assert _verdict(L, L.bn254_dbg_g1_msm(sh, len(good), None, nt, bb, len(bases), 1, None, n, 65536, 0, 0, out, inf, st, info, NO_DEVICE)) == REFUSED
    assert _verdict(L, L.bn254_dbg_g1_msm(sh, len(good), records, nt, bb, len(bases), 1, None, n, 65536, 0, 1, out, inf, None, info, NO_DEVICE)) == REFUSED

    # the row sums
    one = D.encode(D.mont(1))
    row = M.raw_row([one, one, one])

    def rows(r, count_a=1, count_b=0, items=1, fmt=1, mode=0, o=out):
        return _verdict(L, L.bn254_dbg_g1_sum_rows(r, fmt, count_a, count_b, items, mode, o, inf, st, NO_DEVICE))

    assert rows(row) == PAST
    assert rows(row * 32, count_a=30, count_b=2) == PAST
    hi = list(one); hi[3] = (1 << 28) + 1                               # a low digit past 2^28
    lo = list(one); lo[0] = -(1 << 28) - 1
    edge = list(one); edge[7] = 1 << 28                                 # 2^28 itself is inside (what a digit-wise negation leaves)
    big = D.encode(D.mont(5) + 3 * M.P)                                 # above 3 p
    small = D.encode(D.mont(5) - 4 * M.P)
    at3p, atm3p = D.encode(3 * M.P), D.encode(-3 * M.P)                  # the bound itself is inside
    assert rows(M.raw_row([edge, at3p, atm3p])) == PAST
    for what, rc in (("digit above", rows(M.raw_row([hi, one, one]))), ("digit below", rows(M.raw_row([one, lo, one]))), ("value above 3 p", rows(M.raw_row([one, one, big]))),
                     ("value below -3 p", rows(M.raw_row([small, one, one]))), ("3 p + 1", rows(M.raw_row([D.encode(3 * M.P + 1), one, one]))),
                     ("n = 0", rows(row, items=0)), ("n above the cap", rows(row, items=65537)), ("no rows", rows(row, count_a=0)),
                     ("33 rows", rows(row * 33, count_a=33)), ("32 + 1 rows", rows(row * 33, count_a=32, count_b=1)), ("negative count", rows(row, count_b=-1)),
                     ("format", rows(row, fmt=2)), ("mode", rows(row, mode=2)), ("null rows", rows(None)), ("null out", rows(row, o=None)),
                     ("format 0 above p", rows(b"\xff" * 96, fmt=0))):
        assert rc == REFUSED, what

    # the group sums
    g = O.g1_gen()
    nf = C.c_uint()

    def grp(p0, p1, status, items, verdicts=None, so=st):
        return _verdict(L, L.bn254_dbg_plonk_group_sums(p0, p1, status, items, out, out, inf, verdicts, so, C.byref(nf), NO_DEVICE))

    assert grp(g * 65, g * 65, bytes([M.PENDING]) * 65, 65) == PAST
    for what, rc in (("n = 0", grp(g, g, b"\x80", 0)), ("n above the cap", grp(g, g, b"\x80", 65537)), ("null points", grp(None, g, b"\x80", 1)),
                     ("null status", grp(g, g, None, 1)), ("x above p", grp(b"\xff" * 64, g, b"\x80", 1)), ("verdicts without an output", grp(g, g, b"\x80", 1, b"\x01", None))):
        assert rc == REFUSED, what
