"""Value-level GPU tests of the Groth16 loader stage: what the launches before the pairing leave in the workspace -- A, B, C as parsed, L = K_0 + sum x_j K_j and
the status byte -- compared byte for byte with the oracle's, in every form the product launches (probes bn254_dbg_g16_loader, bn254_dbg_g16_loader_keys), and the
sums inside the cooperative kernels (bn254_dbg_coop12_miller_g16; k_coop12_miller_g16_keys by verdict).  Vectors and expectations: tests/g16_loader_common.py."""
import ctypes as C
import os
import random

import pytest

import g16_loader_common as V

pytestmark = pytest.mark.gpu
SEED = 0x61D00
O_MUL = 0      # oracle fp12_op


@pytest.fixture(scope="module")
def dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return 0


@pytest.fixture(scope="module")
def scalars():
    return V.all_scalars()


class Keys:
    """prepared keys of this module by (key bytes, byte windows), closed at the end"""

    def __init__(self, pkg):
        self.pkg, self.made = pkg, {}

    def get(self, vk, byte_windows=False):
        if (vk, byte_windows) not in self.made:
            old = os.environ.get("BN254_WIDE_COMB")
            if byte_windows:
                os.environ["BN254_WIDE_COMB"] = "0"       # read when a key is prepared (tests/test_gpu_rlc_forgery.py::test_groth16_byte_window_tables)
            try:
                self.made[(vk, byte_windows)] = self.pkg.PreparedVk(vk, self.pkg.VK_GNARK)
            finally:
                if byte_windows:
                    os.environ.pop("BN254_WIDE_COMB") if old is None else os.environ.__setitem__("BN254_WIDE_COMB", old)
        return self.made[(vk, byte_windows)]

    def close(self):
        for k in self.made.values():
            k.close()


@pytest.fixture(scope="module")
def keys(pkg):
    k = Keys(pkg)
    yield k
    k.close()


def run_form(pkg, pvk, rows, n_public, form, flags=0, misalign=0, n_used=None):
    """one probe call over `rows`; compares everything the stage leaves with the rows' expectations and returns the probe's report (form, chunks, reduce, tables,
    check_scalars, comb_digits: what bn254_launch_g16_loader recorded at its launch sites)"""
    n = len(rows)
    n_used = n_public if n_used is None else n_used
    want_st = [V.strict_status(r, n_used) if flags & pkg.FLAG_STRICT_SCALARS else r.status for r in rows]
    got = pkg.dbg_g16_loader(pvk, b"".join(r.rec for r in rows), b"".join(r.inputs() for r in rows), n_public, n, form, flags=flags, misalign=misalign)
    assert got["form"] == form and got["check_scalars"] == bool(flags & pkg.FLAG_STRICT_SCALARS and n_public) and got["comb_digits"] == (got["tables"] == "comb")
    if form == pkg.G16_LOADER_COMPACT:
        live = [i for i in range(n) if V.pending(want_st[i])]
        assert list(got["status"]) == [V.PENDING if V.pending(s) else s for s in want_st]            # k_g16_classify: the final byte, or pending
        assert got["slot_proof"] == live + [0xffffffff] * (n - len(live))
        assert list(got["slot_status"]) == [want_st[i] for i in live] + [0] * (n - len(live))
        for j, i in enumerate(live):
            assert got["points"][j] == V.expected_points(rows[i]), (j, i, rows[i].tag)
        return got
    assert list(got["status"]) == want_st, [(i, rows[i].tag, got["status"][i], want_st[i]) for i in range(n) if got["status"][i] != want_st[i]][:8]
    for i in range(n):
        if V.pending(want_st[i]):
            assert got["points"][i] == V.expected_points(rows[i]), (i, rows[i].tag)
    return got


@pytest.fixture(scope="module")
def classes(pkg, O):
    return V.make_classes(pkg, O, SEED + 2, 2)[1]


def lane_rows(pkg, O, classes, width, scalars, replace=None, extra=(), positions=None, seed_salt=0):
    vk = V.key_bytes(pkg, SEED + width, width)
    if replace:
        k = V.key_points(O, vk)
        vk = V.splice_k(O, vk, replace(k))
    ctx = V.KeyCtx(O, vk, SEED + width + seed_salt)
    rows = V.build_rows(ctx, classes, range(width) if positions is None else positions, scalars, extra=extra)
    return vk, ctx, rows


# ---------------------------------------------------------------------------------------------------------------- lane form: k_g16_prepare
@pytest.mark.parametrize("width", [1, 2, 8, 16])
def test_lane_form(pkg, O, dev, keys, classes, scalars, width):
    """k_g16_prepare's window walk at widths 1, 2, 8, 16: every edge scalar in every input position, every loader class, in calls of 257, 65, 64, 63 and 1 proofs;
    plain and on compacted slots; one call with the input rows at an odd byte offset."""
    vk, ctx, rows = lane_rows(pkg, O, classes, width, scalars)
    pvk = keys.get(vk)
    calls = V.cut(rows)
    assert {len(c) for c in calls} >= set(V.SIZES) or width < 8
    for k, call in enumerate(calls):
        for form in (pkg.G16_LOADER_LANES, pkg.G16_LOADER_COMPACT):
            got = run_form(pkg, pvk, call, width, form, misalign=(1 + k % 3) if k % 2 else 0)
            assert (got["chunks"], got["reduce"], got["tables"]) == (0, None, "fw13")
    # all classes in one call: the compaction has decided and pending proofs interleaved
    cls = [r for r in rows if r.tag[0] == "class"]
    assert {V.pending(r.status) for r in cls} == {True, False} and len({r.status for r in cls}) >= 5
    mixed = [x for pair in zip(cls, rows[:len(cls)]) for x in pair] * 6
    run_form(pkg, pvk, mixed[:65], width, pkg.G16_LOADER_COMPACT)


def _degenerate(family):
    """K points replaced, and the rows that meet them: (replace(k) -> {index: point}, extra rows as (background, {position: scalar}, tag))"""
    e = [1, 2, 8191, 8192, V.R - 1, V.R + 1, 2 ** 256 - 1, 0x0123456789abcdef << 64]
    if family == "K2 = K1":
        return (lambda k: {2: k[1]}), [(b, {0: x, 1: x}, ("equal", x)) for b, x in enumerate(e)]
    if family == "K2 = -K1":
        return (lambda k: {2: V.g1_neg(k[1])}), [(b, {0: x, 1: x}, ("opposite", x)) for b, x in enumerate(e)]
    if family == "K1 = K0":
        return (lambda k: {1: k[0]}), [(b, {0: x}, ("K0 doubled", x)) for b, x in enumerate([1, V.R + 1, 2, 3])]
    if family == "K1 = -K0":
        return (lambda k: {1: V.g1_neg(k[0])}), [(b, {0: x}, ("K0 cancelled", x)) for b, x in enumerate([1, V.R + 1, 1, V.R + 1, 2])]
    raise AssertionError(family)


@pytest.mark.parametrize("family", ["K2 = K1", "K2 = -K1", "K1 = K0", "K1 = -K0"])
@pytest.mark.parametrize("width", [2, 16])
def test_lane_form_degenerate_keys(pkg, O, dev, keys, classes, family, width):
    """Equal and opposite summands inside k_g16_prepare's chain of mixed additions: K_2 = +-K_1 with equal scalars, and K_1 = +-K_0 with x_1 = 1 and r + 1 -- the
    accumulator K_0 meets its own table entry (a doubling) or its negative (the identity, mid-chain when later inputs follow; L itself with every other input zero:
    BN254_ST_LINF and the point (0, 1))."""
    replace, extra = _degenerate(family)
    vk, ctx, rows = lane_rows(pkg, O, classes, width, [0, 1], replace=replace, positions=[0, width - 1], seed_salt=7)
    first = len(ctx.bgs)
    for b in range(4):
        ctx.background(zero_from=1 if family.startswith("K1") and b >= 2 else None)      # K1 = +-K0: two backgrounds with every later input zero
    more = []
    for b, over, tag in extra:
        xs, L = ctx.L_override(first + b % 4, over)
        more.append(V.Row(xs, rows[0].rec, L, V.PENDING, tag))
    V.finish(more)
    if family == "K1 = -K0":
        assert sum(r.L is None for r in more) == 2 and all(r.status == V.PENDING | V.LINF for r in more if r.L is None)
    pvk = keys.get(vk)
    for form in (pkg.G16_LOADER_LANES, pkg.G16_LOADER_COMPACT):
        run_form(pkg, pvk, more + rows, width, form)


def test_input_count_mismatch(pkg, O, dev, keys, classes, scalars):
    """n_public passed unequal to the key's width (inputs_match_key = 0): L = K_0, no additions, the byte still pending (the Miller tail makes it INPUT_LEN)."""
    vk = V.key_bytes(pkg, SEED + 2, 2)
    ctx = V.KeyCtx(O, vk, SEED + 99)
    rows = [V.Row([x, scalars[(i * 7) % len(scalars)], 2 ** 256 - 1 - i], rec, ctx.k[0], classes.status(rec), ("mismatch", i))
            for i, (x, (_, rec)) in enumerate(zip(scalars, classes.records * 20))][:65]
    V.finish(rows)
    pvk = keys.get(vk)
    for form in (pkg.G16_LOADER_LANES, pkg.G16_LOADER_COMPACT):
        run_form(pkg, pvk, rows, 3, form)
    run_form(pkg, pvk, rows, 3, pkg.G16_LOADER_LANES, flags=pkg.FLAG_STRICT_SCALARS)          # the strict check counts the inputs as passed


def test_strict_scalars(pkg, O, dev, keys, classes, scalars):
    """BN254_FLAG_STRICT_SCALARS: k_g16_check_scalars after the loader.  Rows with a scalar >= r become NOT_MEMBER, whatever the loader said; the others keep their
    byte and their L.  Lane form (width 2) and wide form (width 17: the partial sums then skip the decided rows)."""
    for width, form in ((2, pkg.G16_LOADER_LANES), (17, pkg.G16_LOADER_WIDE)):
        vk, ctx, rows = lane_rows(pkg, O, classes, width, scalars, positions=[0, width - 1])
        big = sum(any(x >= V.R for x in r.xs) for r in rows)
        assert 0 < big < len(rows) and any(any(x >= V.R for x in r.xs) for r in rows if not V.pending(r.status))
        for call in V.cut(rows)[:3]:
            run_form(pkg, keys.get(vk), call, width, form, flags=pkg.FLAG_STRICT_SCALARS, misalign=2)


# ---------------------------------------------------------------------------------------------------------------- wide forms
_WIDE = {}      # (width, positions) -> the rows of the unmodified key, computed once and shared by the tests of both table forms


def wide_rows(pkg, O, classes, width, scalars, positions, replace=None, same_chunks=None):
    """Rows of a wide key: the scalar rows of `positions` on random and on all-zero backgrounds, the class rows, then whole-chunk rows: one chunk all zero, every
    chunk zero (L = K_0), only the tail chunk live.  same_chunks (a, b): chunk b's scalars are chunk a's in every row (for keys whose chunk b repeats or negates chunk a)."""
    memo = (width, tuple(positions), len(scalars))
    if not replace and memo in _WIDE:
        return _WIDE[memo]
    vk = V.key_bytes(pkg, SEED + width, width)
    if replace:
        vk = V.splice_k(O, vk, replace(V.key_points(O, vk)))
    ctx = V.KeyCtx(O, vk, SEED + 1000 + width)
    chunks = (width + 15) // 16
    extra = [(0, {j: 0 for j in range(16 * c, min(16 * c + 16, width))}, ("zero chunk", c)) for c in sorted({0, 1, chunks - 1, 8 % chunks, 9 % chunks})]
    extra.append((1, {j: 0 for j in range(width)}, ("all zero",)))
    extra.append((0, {j: 0 for j in range(16 * (chunks - 1))}, ("only the tail chunk",)))
    rows = V.build_rows(ctx, classes, positions, scalars, n_bg=4, zero_bg=True, extra=extra)
    if same_chunks:
        a, b = same_chunks
        for r in rows:
            over = {16 * b + t: r.xs[16 * a + t] for t in range(16)}
            r.xs = [over.get(j, x) for j, x in enumerate(r.xs)]
            r.L = ctx.L_of(r.xs)
            r.status &= ~V.LINF
        V.finish(rows)
    assert any(r.tag == ("all zero",) and r.L == ctx.k[0] for r in rows) or same_chunks
    if not replace:
        _WIDE[memo] = (vk, ctx, rows, chunks)
    return vk, ctx, rows, chunks


def run_wide(pkg, pvk, rows, width, chunks, forms, tables):
    calls = V.cut(rows)
    for k, call in enumerate(calls):
        if len(call) > 32:
            assert call[31].xs != call[32].xs          # k_g16_msm_reduce8: the last proof of a block of 32 and the first of the next carry different rows
        for form in forms:
            got = run_form(pkg, pvk, call, width, form, misalign=(k % 4))
            assert (got["chunks"], got["reduce"], got["tables"]) == (chunks, "k_g16_msm_reduce8" if form == pkg.G16_LOADER_WIDE8 else "k_g16_msm_reduce", tables)


def _positions(width):
    """every position up to width 33; at 241 and 256 the ends of the first, second, ninth and last chunks (chunk 8 is the first a lane of k_g16_msm_reduce8 adds second)"""
    return list(range(width)) if width <= 33 else sorted({0, 15, 16, 128, 143, 16 * ((width - 1) // 16), width - 1})


@pytest.mark.parametrize("width", [17, 32, 33, 241, 256])
def test_wide_comb(pkg, O, dev, keys, classes, scalars, width):
    """k_g16_comb_digits -> k_g16_msm_partial_comb -> k_g16_msm_reduce, and from 16 chunks on k_g16_msm_reduce8 on the same key: widths 17 (a tail chunk of one input),
    32 and 33 (the first full-chunk boundary), 241 (16 chunks, a one-input tail) and 256."""
    vk, ctx, rows, chunks = wide_rows(pkg, O, classes, width, scalars, _positions(width))
    forms = [pkg.G16_LOADER_WIDE] + ([pkg.G16_LOADER_WIDE8] if chunks >= 16 else [])
    assert (chunks >= 16) == (width >= 241)
    run_wide(pkg, keys.get(vk), rows, width, chunks, forms, "comb")
    if chunks < 16:
        with pytest.raises(pkg.Bn254Error):
            pkg.dbg_g16_loader(keys.get(vk), rows[0].rec, rows[0].inputs(), width, 1, pkg.G16_LOADER_WIDE8)


@pytest.mark.parametrize("width", [17, 33])
def test_wide_byte_windows(pkg, O, dev, keys, classes, scalars, width):
    """k_g16_msm_partial, the byte windows of a key prepared under BN254_WIDE_COMB=0."""
    vk, ctx, rows, chunks = wide_rows(pkg, O, classes, width, scalars, _positions(width))
    run_wide(pkg, keys.get(vk, byte_windows=True), rows, width, chunks, [pkg.G16_LOADER_WIDE], "bytes")


@pytest.mark.parametrize("family,width,pair", [("equal", 33, (0, 1)), ("opposite", 33, (0, 1)), ("equal", 256, (0, 8)), ("opposite", 256, (0, 8))])
def test_wide_equal_and_opposite_chunks(pkg, O, dev, keys, classes, scalars, family, width, pair):
    """Two chunks whose sums are equal, and two whose sums are opposite: 16 K points repeated (negated) and both chunks given the same scalars.  Inside a chunk every
    comb column then adds the same point twice (a doubling in g1_add_mixed) or a point and its negative (the identity mid-chain); at width 256 chunks 0 and 8 are
    the two a lane of k_g16_msm_reduce8 adds first (a doubling, or the identity, in g1_add on re-loaded rows)."""
    a, b = pair
    sign = (lambda p: p) if family == "equal" else V.g1_neg
    def replace(k):
        # inside one chunk as well: K_2 = +-K_1 (equal scalars in positions 0 and 1 of some rows, below)
        k = list(k); k[2] = sign(k[1])
        return {2: k[2], **{1 + 16 * b + t: sign(k[1 + 16 * a + t]) for t in range(16)}}

    vk, ctx, rows, chunks = wide_rows(pkg, O, classes, width, scalars[:40], [0, 15], replace=replace, same_chunks=pair)
    for r in rows[::3]:
        r.xs[1] = r.xs[0]; r.xs[16 * b + 1] = r.xs[16 * b]
        r.L = ctx.L_of(r.xs); r.status &= ~V.LINF
    V.finish(rows)
    if family == "opposite":
        assert all(V.g1_add(O, ctx.term(16 * a + t, 5), ctx.term(16 * b + t, 5)) is None for t in (0, 15))
    forms = [pkg.G16_LOADER_WIDE] + ([pkg.G16_LOADER_WIDE8] if chunks >= 16 else [])
    run_wide(pkg, keys.get(vk), rows, width, chunks, forms, "comb")


# ---------------------------------------------------------------------------------------------------------------- the cooperative kernels
def _g2_neg(q):
    return q[:64] + V.be((V.P - int.from_bytes(q[64:96], "big")) % V.P) + V.be((V.P - int.from_bytes(q[96:128], "big")) % V.P)


@pytest.mark.parametrize("width", [2, 16])
def test_coop12_miller_g16_edge_scalars(pkg, O, dev, keys, classes, scalars, width):
    """k_coop12_miller_g16's own sum (L stays projective in the kernel): the GT value it stores is e(A, B) e(L, -gamma) e(C, -delta) with L from the oracle, for the
    edge scalar rows at widths 2 (both positions) and 16.  The kernel deals the windows of input j to its twelve lanes from offset 20 j mod 12, which takes the
    values 0, 8 and 4: at width 16 every scalar goes through positions 0 and 15 (offset 0), 7 (offset 8) and 2 (offset 4)."""
    lib = pkg.lib()
    lib.bn254_dbg_coop12_miller_g16.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    vk, ctx, rows = lane_rows(pkg, O, classes, width, scalars, positions=range(width) if width == 2 else [0, 2, 7, 15])
    assert width == 2 or {20 * j % 12 for j in (0, 2, 7, 15)} == {20 * j % 12 for j in range(16)}
    rows = [r for r in rows if r.tag[0] == "scalar"]
    dec2 = lambda b: O.decompress_g2(b, O.MODE_GNARK)[1]
    neg_gamma, neg_delta = _g2_neg(dec2(vk[128:192])), _g2_neg(dec2(vk[224:288]))
    rec = rows[0].rec
    fixed = O.pairing(rec[0:64] + rec[192:256], rec[64:192] + neg_delta)
    n = len(rows)
    out, st = (C.c_uint8 * (384 * n))(), (C.c_uint8 * n)()
    assert lib.bn254_dbg_coop12_miller_g16(keys.get(vk).handle, b"".join(r.rec for r in rows), b"".join(r.inputs() for r in rows), width, n, out, st, dev) == 0
    out = bytes(out)
    assert list(bytes(st)) == [O.ACCEPT] * n
    for i, r in enumerate(rows):
        want = fixed if r.L is None else O.fp12_op(O_MUL, fixed, O.pairing(r.L, neg_gamma))
        assert out[384 * i:384 * i + 384] == want, (i, r.tag)


# ---------------------------------------------------------------------------------------------------------------- key lists
KEY_WIDTHS = (1, 2, 5)
KEY_STRIDE = 32 * 7                 # wider than the widest key


def key_list_batch(pkg, O, classes, scalars):
    """three keys of widths 1, 2, 5; per key ALL its rows -- every scalar in every input position, and the class rows -- under a shuffled key_index.  Returns the key
    bytes, the batch as (key, row) and the rows per key: 178, 342 and 834, none a multiple of 64, so every key's last granule is partly padding."""
    rng = random.Random(SEED + 5)
    per_key = []
    for kk, w in enumerate(KEY_WIDTHS):
        vk = V.key_bytes(pkg, SEED + 40 + w, w)
        ctx = V.KeyCtx(O, vk, SEED + 50 + w)
        rows = V.build_rows(ctx, classes, range(w), scalars)
        assert {(r.tag[1], r.tag[2]) for r in rows if r.tag[0] == "scalar"} == {(j, x) for j in range(w) for x in scalars}      # nothing cut
        assert all(r.xs[r.tag[1]] == r.tag[2] for r in rows if r.tag[0] == "scalar") and len(rows) % 64 != 0
        per_key.append((vk, rows))
    order = [kk for kk, (_, rows) in enumerate(per_key) for _ in rows]
    rng.shuffle(order)
    it = [iter(rows) for _, rows in per_key]
    batch = [(kk, next(it[kk])) for kk in order]
    return [vk for vk, _ in per_key], batch, [len(rows) for _, rows in per_key]


def test_key_list_loader(pkg, O, dev, keys, classes, scalars):
    """k_g16_prepare_keys (byte windows of the set's tables, the key per wavefront, the slot -> proof map, input_stride): every slot's A, B, C, L and status byte are the
    oracle's for the proof the slot map names; padding slots have status 0.  The bytes behind a narrow key's inputs are 0xff: never summed, never counted by the
    strict check.  Rows at an aligned and at an odd address."""
    vks, batch, counts = key_list_batch(pkg, O, classes, scalars)
    assert len(batch) == sum(counts) == sum(len(scalars) * w + len(classes.records) for w in KEY_WIDTHS)
    ks = pkg.KeySet([keys.get(vk) for vk in vks])
    index = [kk for kk, _ in batch]
    proofs = b"".join(r.rec for _, r in batch)
    inputs = b"".join(r.inputs(KEY_STRIDE, 0xff) for _, r in batch)
    for flags, misalign in ((0, 0), (0, 3), (pkg.FLAG_STRICT_SCALARS, 1)):
        got = pkg.dbg_g16_loader_keys(ks, index, proofs, inputs, flags=flags, misalign=misalign, input_stride=KEY_STRIDE)
        slots = sum((c + 63) // 64 * 64 for c in counts)
        assert got["n_slots"] == slots == len(got["slot_proof"])
        named = [p for p in got["slot_proof"] if p is not None]
        assert sorted(named) == list(range(len(batch)))
        for g in range(slots // 64):                                   # a granule belongs to one key, proofs first
            sl = got["slot_proof"][64 * g:64 * g + 64]
            live = [p for p in sl if p is not None]
            assert live and sl[:len(live)] == live and len({index[p] for p in live}) == 1
        for j, p in enumerate(got["slot_proof"]):
            if p is None:
                assert got["slot_status"][j] == 0, j
                continue
            kk, r = batch[p]
            want = V.strict_status(r, KEY_WIDTHS[kk]) if flags else r.status
            assert got["slot_status"][j] == want, (j, p, r.tag)
            if V.pending(want):
                assert got["points"][j] == V.expected_points(r), (j, p, r.tag)


def test_key_list_direct_form_accepts_edge_rows(pkg, O, dev, keys, scalars):
    """k_coop12_miller_g16_keys has no store mode: it is seen by verdict.  Valid proofs for the edge rows of the three keys -- every scalar in every input position
    of its key, the other positions holding other scalars of the list -- in one batch that takes the direct form come back ACCEPT (a wrong L would REJECT)."""
    rng = random.Random(SEED + 6)
    recs, rows_in, index, pvks = [], [], [], []
    for kk, w in enumerate(KEY_WIDTHS):
        rows = [[scalars[(i + 3 * j + 1) % len(scalars)] if j != pos else scalars[i] for j in range(w)] for pos in range(w) for i in range(len(scalars))]
        assert {(pos, xs[pos]) for pos in range(w) for xs in rows[pos * len(scalars):(pos + 1) * len(scalars)]} == {(pos, x) for pos in range(w) for x in scalars}
        raw = b"".join(V.be(x) for xs in rows for x in xs)
        vk, proofs = pkg.synth_groth16_for_inputs(SEED + 40 + w, w, raw, threads=4)
        pvks.append(keys.get(vk))
        for i, xs in enumerate(rows):
            recs.append((kk, proofs[256 * i:256 * i + 256], b"".join(V.be(x) for x in xs).ljust(KEY_STRIDE, b"\xff")))
    rng.shuffle(recs)
    ks = pkg.KeySet(pvks)
    n = len(recs)
    assert n == len(scalars) * sum(KEY_WIDTHS)
    st = ks.verify_batch([k for k, _, _ in recs], b"".join(p for _, p, _ in recs), b"".join(i for _, _, i in recs), input_stride=KEY_STRIDE, device=dev)
    assert ks.last_form(dev) == 1                       # the direct form: k_g16_prepare + k_coop12_miller_g16_keys
    assert list(st) == [pkg.ACCEPT] * n
