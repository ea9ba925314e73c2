"""Value-level GPU tests of the G1 layer under the PlonK path (csrc/bn254_k_msm.hip): the rows of a multi-scalar multiplication (k_g1_msm_rows,
k_g1_msm_rows_keys), the row sum (k_g1_sum_affine) and the group sums of BN254_FLAG_RLC (k_plonk_group_sums, k_plonk_group_scatter), each through the launcher
the product calls (probes bn254_dbg_g1_msm, bn254_dbg_g1_sum_rows, bn254_dbg_plonk_group_sums).  Everything is bit-exact: the expected points come from the CPU
oracle and from Python integers (tests/msm_records.py), never from another run of the code under test, and every item of a call holds different values.
tests/test_msm_records_cpu.py runs the cases of the first group through the host compile of the same row code: a case that fails here and passes there is a
device-only fault."""
import ctypes as C
import random

import pytest

import msm_records as M

pytestmark = pytest.mark.gpu
P, R, ID = M.P, M.R, M.ID
PENDING, LINF, LINF2, ACCEPT, REJECT, NOT_ON_CURVE = M.PENDING, M.LINF, M.LINF2, M.ACCEPT, M.REJECT, M.NOT_ON_CURVE
STORED_IDENTITY = M.be(0) + M.be(1)          # what the workspace holds for an identity sum
TWO_SUM_CASES = [c[0] for c in M.all_cases() if len(c[1]) == 2]


def _chk(L, rc):
    assert rc == 0, L.bn254_last_error()


@pytest.fixture(scope="module")
def L(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    lib = pkg.lib()
    lib.bn254_dbg_g1_msm.argtypes = [C.POINTER(C.c_int), C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint), C.c_size_t, C.c_size_t,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]
    lib.bn254_dbg_g1_sum_rows.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.bn254_dbg_plonk_group_sums.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_uint), C.c_int]
    return lib


@pytest.fixture(scope="module")
def multiples(O):
    """m G for |m| <= 4096: built once, shared, never modified"""
    return M.Multiples(O)


def _split(buf, size):
    b = bytes(buf)
    return [b[size * i:size * (i + 1)] for i in range(len(b) // size)]


def msm(L, sums, n_terms, records, key_bases, granule_key, n, budget, joint_g, mode, status=None):
    """bn254_dbg_g1_msm: mode 0 -> (points[i][s] with ID for a flagged identity, info); mode 1 -> (stored points[i][0..1], status bytes, info)"""
    sh = M.shape_ints(sums)
    n_keys, n_bases = len(key_bases), len(key_bases[0])
    bb = b"".join(b"".join(kb) for kb in key_bases)
    gk = (C.c_uint * len(granule_key))(*granule_key) if granule_key else None
    info = (C.c_int * 6)()
    k = len(sums) if mode == 0 else 2
    out, inf = (C.c_uint8 * (64 * k * n))(*([0xEE] * (64 * k * n))), (C.c_uint8 * (k * n))(*([0xEE] * (k * n)))
    st = (C.c_uint8 * n)(*status) if mode else None
    _chk(L, L.bn254_dbg_g1_msm(sh, len(sh), records, n_terms, bb, n_bases, n_keys, gk, n, budget, joint_g, mode, out, inf, st, info, 0))
    pts = _split(out, 64)
    if mode:
        return [pts[2 * i:2 * i + 2] for i in range(n)], bytes(st), list(info)
    flags = bytes(inf)
    assert set(flags) <= {0, 1}
    assert all(pts[j] == ID for j in range(k * n) if flags[j]), "a flagged identity must come back as zero bytes"
    return [[ID if flags[k * i + s] else pts[k * i + s] for s in range(k)] for i in range(n)], list(info)


def _run_case(L, c, mode, status=None):
    kb = c["key_bases"] if c["granule_key"] else [c["bases"]]
    return msm(L, c["sums"], c["n_terms"], c["records"], kb, c["granule_key"], c["n"], c["budget"], c["joint_g"], mode, status)


def _diff(got, want):
    return [(i, s) for i in range(len(want)) for s in range(len(want[i])) if got[i][s] != want[i][s]]


# ---------------------------------------------------------------------------------------------------------------- rows and sums together
@pytest.mark.parametrize("name", M.case_names())
def test_msm_values(L, O, name):
    """One launch of the rows kernel and the row sum in the words form, for every plan form, shape, item count, chosen scalar and chosen point of
    tests/msm_records.py; `keys`: k_g1_msm_rows_keys over three keys, every item against the tables of its granule's key."""
    c = M.build_case(L, O, name)
    got, info = _run_case(L, c, 0)
    assert info[4] == c["form"], (name, info)
    assert info[0] == info[2] + info[3] <= M.MAX_ROWS
    bad = _diff(got, c["want"])
    assert not bad, (name, info, bad[:8])


@pytest.mark.parametrize("name", TWO_SUM_CASES)
def test_msm_workspace_and_status(L, O, name):
    """The call of the second PlonK launch: both sums in ONE launch of k_g1_sum_affine, to the workspace, the identity flags OR-ed into the status bytes.  The
    caller's bytes cycle through PENDING, PENDING | 3, ACCEPT, REJECT, NOT_ON_CURVE; in the `points` cases items 8 .. 11 fill one status word with pending bytes
    whose sums are the identity (item 10: both).  A flag lands in pending bytes only; every other byte stays; an identity is stored as (0, 1)."""
    c = M.build_case(L, O, name)
    st = M.status_in(c["n"])
    pts, got_st, info = _run_case(L, c, 1, st)
    assert info[4] == c["form"]
    want_pts = [[STORED_IDENTITY if w == ID else w for w in ws] for ws in c["want"]]
    bad = _diff(pts, want_pts)
    assert not bad, (name, bad[:8])
    want_st = bytes(s | (LINF if w[0] == ID else 0) | (LINF2 if w[1] == ID else 0) if s & PENDING else s for s, w in zip(st, c["want"]))
    assert got_st == want_st, (name, [(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(got_st, want_st)) if a != b][:8])
    if c["what"] == "points":
        assert [got_st[i] for i in (8, 9, 10, 11)] == [PENDING | LINF, PENDING | 3 | LINF2, PENDING | LINF | LINF2, PENDING | 3 | LINF]


def test_msm_keys_cross_reading(L, O):
    """The key-list case once more through the single-key kernel, granule by granule with that granule's bases: the same points as the key-list kernel gave (a
    second reading of the expectation, which stays the oracle's)."""
    c = M.build_case(L, O, "keys")
    multi, _ = _run_case(L, c, 0)
    nt = c["n_terms"]
    for g, k in enumerate(c["granule_key"]):
        lo, hi = 64 * g, min(64 * g + 64, c["n"])
        got, _ = msm(L, c["sums"], nt, c["records"][129 * nt * lo:129 * nt * hi], [c["key_bases"][k]], None, hi - lo, c["budget"], c["joint_g"], 0)
        assert got == multi[lo:hi] == c["want"][lo:hi], g
    # with the granules' keys rotated the fixed terms read other tables: the points must move (the key index is really used)
    rot = [(k + 1) % 3 for k in c["granule_key"]]
    moved, _ = msm(L, c["sums"], nt, c["records"], c["key_bases"], rot, c["n"], c["budget"], c["joint_g"], 0)
    assert all(moved[i] != c["want"][i] for i in range(c["n"]))


# ---------------------------------------------------------------------------------------------------------------- row sums alone
ROW_KINDS = 10


def _row_multipliers(rng, kind, counts):
    """the multipliers of one item's rows, per sum, with the exceptional case `kind` placed in them.  Lane q of the four-lane form adds rows q, q + 4, ...; the
    one-lane form adds them in order.  |m| <= 250 before the adjustments, at most 3750 after: inside the table."""
    out = []
    for count in counts:
        m = [rng.randrange(-250, 251) or 7 for _ in range(count)]
        lane = lambda q: sum(m[q::4])
        if kind in (1, 2) and count > 1:                  # identity rows: (0 : 1 : 0) / (0 : y : 0)
            for r in rng.sample(range(count), max(1, count // 3)):
                m[r] = 0
        elif kind == 3:                                   # equal rows that meet in a lane's own loop (rows 0 and 1 for one lane, rows 0 and 4 for four)
            for r in (1, 4):
                if r < count:
                    m[r] = m[0]
        elif kind == 4 and count > 1:                     # equal partial sums in the FIRST butterfly step: lanes 0 and 1
            m[1] += lane(0) - lane(1)
        elif kind == 5 and count > 2:                     # ... in the SECOND: lanes 0 + 1 against lanes 2 + 3
            m[2] += lane(0) + lane(1) - lane(2) - lane(3)
        elif kind == 6:                                   # opposite rows, in the loop of one lane and of four
            for r in (1, 4):
                if r < count:
                    m[r] = -m[0]
        elif kind == 7:                                   # a total of zero
            m[-1] -= sum(m)
        elif kind == 8 and count > 1:                     # opposite partial sums in the first butterfly step
            m[1] -= lane(0) + lane(1)
        elif kind == 9:                                   # every row the identity
            m = [0] * count
        out.append(m)
    return out


def _rows_case(multiples, rng, counts, n):
    """rows[r][i] as format-0 bytes and the expected sums: item i holds the exceptional case i % ROW_KINDS.  Every other item carries Z != 1, and the choice turns
    over with each round of the kinds (ROW_KINDS is even: by i's parity alone a kind would only ever meet one form of Z), so from n = 2 ROW_KINDS on every kind runs
    with Z = 1 and with scaled coordinates"""
    ms = [_row_multipliers(rng, i % ROW_KINDS, counts) for i in range(n)]
    scaled = lambda i: (i + i // ROW_KINDS) & 1
    rows = []
    for s, count in enumerate(counts):
        for r in range(count):
            rows.append([M.proj_row(multiples, ms[i][s][r], rng if scaled(i) else None, 1 if i % ROW_KINDS != 2 else rng.randrange(2, P)) for i in range(n)])
    want = [[multiples(sum(ms[i][s])) for s in range(len(counts))] for i in range(n)]
    return rows, want


def sum_rows(L, rows, fmt, counts, n, mode, status=None):
    count_a, count_b = counts[0], counts[1] if len(counts) > 1 else 0
    k = len(counts) if mode == 0 else 2
    out, inf = (C.c_uint8 * (64 * k * n))(*([0xEE] * (64 * k * n))), (C.c_uint8 * (k * n))(*([0xEE] * (k * n)))
    st = (C.c_uint8 * n)(*status) if mode else None
    _chk(L, L.bn254_dbg_g1_sum_rows(b"".join(b"".join(r) for r in rows), fmt, count_a, count_b, n, mode, out, inf, st, 0))
    pts = _split(out, 64)
    if mode:
        return [pts[2 * i:2 * i + 2] for i in range(n)], bytes(st)
    flags = bytes(inf)
    assert set(flags) <= {0, 1} and all(pts[j] == ID for j in range(k * n) if flags[j])
    return [[ID if flags[k * i + s] else pts[k * i + s] for s in range(k)] for i in range(n)]


def _check_rows(L, multiples, rng, counts, n, fmt=0, rows_want=None):
    rows, want = rows_want or _rows_case(multiples, rng, counts, n)
    got = sum_rows(L, rows, fmt, counts, n, 0)
    bad = _diff(got, want)
    assert not bad, (counts, n, "words", bad[:8])
    if len(counts) == 2:                                  # the two sums in ONE launch, split at round_up(n, 64): the workspace form
        st = bytes(M.STATUS_CYCLE[i % 5] if i % 4 != 2 else PENDING for i in range(n))
        pts, got_st = sum_rows(L, rows, fmt, counts, n, 1, st)
        bad = _diff(pts, [[STORED_IDENTITY if w == ID else w for w in ws] for ws in want])
        assert not bad, (counts, n, "workspace", bad[:8])
        want_st = bytes(s | (LINF if w[0] == ID else 0) | (LINF2 if w[1] == ID else 0) if s & PENDING else s for s, w in zip(st, want))
        assert got_st == want_st, (counts, n, [(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(got_st, want_st)) if a != b][:8])


@pytest.mark.parametrize("counts", [(1,), (3,), (4,), (5,), (14,), (14, 2), (4, 1)])
def test_sum_rows_forms(L, multiples, counts):
    """Fewer than four rows: one lane per item; four or more: four lanes and two butterfly steps.  n = 70: the last wavefront is partly dead in both forms.  Identity
    rows, equal rows in a lane's loop and in either butterfly step, opposite rows, a total of zero, Z != 1 -- placed by the multipliers."""
    _check_rows(L, multiples, random.Random("rows-%r" % (counts,)), counts, 70)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sum_rows_item_counts(L, multiples, n):
    rng = random.Random("rows-n%d" % n)
    _check_rows(L, multiples, rng, (5,), n)
    _check_rows(L, multiples, rng, (4, 1), n)


@pytest.mark.parametrize("counts,n", [((4, 1), 8192), ((4, 1), 8193), ((4,), 16384), ((4,), 16385)])
def test_sum_rows_lane_form_handover(L, multiples, counts, n):
    """bn254_launch_g1_sum_rows takes four lanes per item while the launch stays within 65 536 lanes: up to 16 384 items with one sum, 8192 with two; one more item
    is the one-lane form.  Every item differs; the last items decide whether the grid covers them."""
    _check_rows(L, multiples, random.Random("rows-%r-%d" % (counts, n)), counts, n)


@pytest.mark.parametrize("count", [3, 5])
def test_sum_rows_representatives(L, O, multiples, count):
    """Format 1: the caller's digits reach the additions as they are.  Every coordinate of every row as m, m +- p, m +- 2 p and as the largest and the smallest
    representative inside +-3 p (what k_g1_sum_affine declares for a row); X with the digit patterns of fp12_digits.pattern.  The affine sum is that of the
    canonical representatives."""
    rng = random.Random("rows-reps-%d" % count)
    n = 70
    ms = [[rng.randrange(-290, 291) or 7 for _ in range(count)] for _ in range(n)]
    rows = []
    for r in range(count):
        row = []
        for i in range(n):
            x, y = multiples.xy(ms[i][r])
            z = rng.randrange(2, P) if i & 1 else 1
            co = [x * z % P, y * z % P, z]
            if i % 7 == 6:
                row.append(M.raw_row([M.extreme_rep(v, (i // 7 + r + c) & 1) for c, v in enumerate(co)]))
            else:
                row.append(M.raw_row([M.rep_digits(v, (i + r + 2 * c) % 5 - 2) for c, v in enumerate(co)]))
        rows.append(row)
    want = [[multiples(sum(ms[i]))] for i in range(n)]
    _check_rows(L, multiples, rng, (count,), n, fmt=1, rows_want=(rows, want))
    # the digit patterns: the same point in every row, so the sum is count P (doublings along the way); the other coordinates vary their representative
    pats = [M.pattern_point(kind, rng) for kind in range(4)]
    n = len(pats)
    rows = [[M.raw_row([d, M.rep_digits(y, (r + i) % 5 - 2), M.rep_digits(1, (2 * r + i) % 5 - 2)]) for i, (d, x, y) in enumerate(pats)] for r in range(count)]
    want = [[O.g1_mul(M.be(x) + M.be(y), count)] for d, x, y in pats]
    _check_rows(L, multiples, rng, (count,), n, fmt=1, rows_want=(rows, want))


# ---------------------------------------------------------------------------------------------------------------- group sums
GROUP_KINDS = ["all-pending", "none-pending", "one-pending", "scattered", "all-same", "cancel0", "cancel-both"] + ["pair-%d" % m for m in (1, 2, 4, 8, 16, 32)]
DECIDED = [ACCEPT, REJECT, NOT_ON_CURVE, 2, 5]


def _group(rng, kind, size):
    """one group of `size` proofs: (status bytes, multipliers of P0, of P1); a multiplier of None stands for junk under an identity flag or a decided byte"""
    st = [PENDING] * size
    m0 = [rng.randrange(-60, 61) or 3 for _ in range(size)]
    m1 = [rng.randrange(-60, 61) or 5 for _ in range(size)]
    if kind == "none-pending":
        st = [DECIDED[(j + size) % len(DECIDED)] for j in range(size)]
    elif kind == "one-pending":
        keep = rng.randrange(size)
        st = [PENDING if j == keep else DECIDED[j % len(DECIDED)] for j in range(size)]
    elif kind == "scattered":                             # decided proofs and flagged proofs through the group: neither may count
        for j in range(size):
            st[j] = [PENDING, DECIDED[j % len(DECIDED)], PENDING | LINF, PENDING, PENDING | LINF2, PENDING | LINF | LINF2, PENDING][j % 7]
    elif kind == "all-same":                              # every butterfly step doubles: 64 P
        a, b = rng.randrange(1, 65), -rng.randrange(1, 65)
        m0, m1 = [a] * size, [b] * size
    elif kind.startswith("pair-"):                        # lanes j and j xor m hold the same point: the step with that mask adds equal sums
        m = int(kind[5:])
        f0 = [rng.randrange(-60, 61) or 3 for _ in range(64)]
        f1 = [rng.randrange(-60, 61) or 5 for _ in range(64)]
        m0, m1 = [f0[j & ~m] for j in range(size)], [f1[j & ~m] for j in range(size)]
    def cancel(m):                                        # the last multiplier takes the rest; no multiplier may become 0 (a finite point stands for it)
        while True:
            m[-1] -= sum(m)
            if m[-1]:
                return
            m[0] += 1
    if kind in ("cancel0", "cancel-both") and size > 1:
        cancel(m0)
    if kind == "cancel-both" and size > 1:
        cancel(m1)
    return st, m0, m1


def _groups_case(multiples, rng, n, first_kind):
    st, p0, p1, want = [], [], [], []
    for g in range((n + 63) // 64):
        size = min(64, n - 64 * g)
        kind = GROUP_KINDS[(first_kind + g) % len(GROUP_KINDS)]
        s, m0, m1 = _group(rng, kind, size)
        t0 = t1 = 0
        for j in range(size):
            pend = bool(s[j] & PENDING)
            use0, use1 = pend and not s[j] & LINF, pend and not s[j] & LINF2
            assert m0[j] and m1[j]
            p0.append(multiples(m0[j]) if use0 else M.junk_point(rng))          # junk under an identity flag and under a decided byte: it must not count
            p1.append(multiples(m1[j]) if use1 else M.junk_point(rng))
            t0 += m0[j] if use0 else 0
            t1 += m1[j] if use1 else 0
        st += s
        if any(x & PENDING for x in s):
            want.append((multiples(t0), multiples(t1), PENDING | (0 if t0 else LINF) | (0 if t1 else LINF2)))
        else:
            want.append((ID, ID, ACCEPT))
    return bytes(st), b"".join(p0), b"".join(p1), want


def group_sums(L, p0, p1, st, n, verdicts=None):
    groups = (n + 63) // 64
    o0, o1, gs = (C.c_uint8 * (64 * groups))(), (C.c_uint8 * (64 * groups))(), (C.c_uint8 * groups)(*([0xEE] * groups))
    so, nf = (C.c_uint8 * n)(*([0xEE] * n)), C.c_uint(0xEEEE)
    _chk(L, L.bn254_dbg_plonk_group_sums(p0, p1, st, n, o0, o1, gs, verdicts, so, C.byref(nf), 0))
    return _split(o0, 64), _split(o1, 64), bytes(gs), bytes(so), nf.value


GROUP_CASES = [(1, 0), (64, 4), (65, 5), (200, 0), (200, 7), (1030, 0), (200, 3), (192, 1), (448, 6)]
VERDICTS = [ACCEPT, PENDING, ACCEPT, ACCEPT, PENDING | LINF, REJECT, ACCEPT]
SCATTERED_VERDICTS = [PENDING, PENDING | LINF, ACCEPT]    # a scattered group is the only one whose pending bytes carry flags on input: it must meet failed verdicts
FLAGGED = {PENDING | LINF, PENDING | LINF2, PENDING | LINF | LINF2}


def _group_kind(g, first_kind):
    return GROUP_KINDS[(first_kind + g) % len(GROUP_KINDS)]


def _verdict(g, first_kind):
    """the verdict the test hands the scatter for group g: passed and failed (still pending, pending with an identity flag, rejected) in turn; for a scattered
    group chosen by kind, so that flagged pending bytes meet a failed verdict of either pending form, and a passed one"""
    if _group_kind(g, first_kind) == "scattered":
        return SCATTERED_VERDICTS[g % 3]
    return VERDICTS[(g + first_kind) % len(VERDICTS)]


def _scattered_groups():
    """(n, first_kind, g, size, verdict) of every scattered group of GROUP_CASES"""
    return [(n, fk, g, min(64, n - 64 * g), _verdict(g, fk)) for n, fk in GROUP_CASES for g in range((n + 63) // 64) if _group_kind(g, fk) == "scattered"]


# all three flagged bytes need a group of at least six proofs; each verdict of SCATTERED_VERDICTS must meet such a group, and every kind a FULL group in a
# case of its own beside [1030-0]
assert {v for _, _, _, size, v in _scattered_groups() if size >= 6} == set(SCATTERED_VERDICTS)
assert all(sum(1 for n, fk in GROUP_CASES for g in range(n // 64) if _group_kind(g, fk) == kind) >= 2 for kind in GROUP_KINDS)


@pytest.mark.parametrize("n,first_kind", GROUP_CASES)
def test_group_sums_and_scatter(L, multiples, n, first_kind):
    """k_plonk_group_sums: per group of 64 proofs the sum of the points of its pending proofs, six butterfly steps of complete additions.  Groups in turn: every
    proof pending; none (status ACCEPT); one; decided and identity-flagged proofs scattered through the group with junk for points; all 64 the same point (every
    step doubles); the same point in lanes j and j xor m for each of the six masks; sums that cancel in P0, and in both.  n = 65, 200 and 1030 end in a partial
    group; [448-6] holds the cancel-both group and the six masks in full groups, [192-1] and [200-3] the first four kinds.  Then k_plonk_group_scatter with
    verdicts the test supplies: pending proofs of passed groups become ACCEPT, flagged ones too ([192-1]); pending proofs of failed groups keep their byte, the
    identity flags of a scattered group included, under a verdict of PENDING ([200-0], [200-3], [1030-0]) and of PENDING | LINF ([1030-0]); decided proofs keep
    theirs; n_failed counts each failed group once."""
    rng = random.Random("groups-%d-%d" % (n, first_kind))
    st, p0, p1, want = _groups_case(multiples, rng, n, first_kind)
    groups = len(want)
    verdicts = bytes(_verdict(g, first_kind) for g in range(groups))
    g0, g1, gs, st_after, n_failed = group_sums(L, p0, p1, st, n, verdicts)
    for g, (w0, w1, ws) in enumerate(want):
        kind = _group_kind(g, first_kind)
        assert gs[g] == ws, (g, kind, hex(gs[g]), hex(ws))
        assert g0[g] == (STORED_IDENTITY if w0 == ID else w0), (g, kind, "P0")
        assert g1[g] == (STORED_IDENTITY if w1 == ID else w1), (g, kind, "P1")
    want_after = bytes(ACCEPT if s & PENDING and verdicts[i // 64] == ACCEPT else s for i, s in enumerate(st))
    assert st_after == want_after, [(i, hex(a), hex(b), hex(verdicts[i // 64])) for i, (a, b) in enumerate(zip(st_after, want_after)) if a != b][:8]
    assert n_failed == sum(1 for v in verdicts if v != ACCEPT)
    for _, _, g, size, v in [c for c in _scattered_groups() if c[:2] == (n, first_kind)]:
        before, after = st[64 * g:64 * g + size], st_after[64 * g:64 * g + size]
        assert size < 6 or FLAGGED <= set(before), (g, "the scattered group must hold every flagged pending byte")
        if v != ACCEPT:                                   # a failed group: the exact check runs on these proofs next and reads their flags
            assert after == before, (g, hex(v))
        else:
            assert all(a == (ACCEPT if b & PENDING else b) for a, b in zip(after, before)), g


def test_group_sums_without_scatter_leave_the_status(L, multiples):
    rng = random.Random("groups-plain")
    st, p0, p1, want = _groups_case(multiples, rng, 130, 3)
    g0, g1, gs, st_after, n_failed = group_sums(L, p0, p1, st, 130)
    assert [x for x in gs] == [w[2] for w in want]
    assert st_after == bytes([0xEE] * 130) and n_failed == 0xEEEE           # nothing ran after the sums: the outputs of the scatter are untouched
