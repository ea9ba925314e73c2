"""The vectors of the loader-stage value tests (tests/g16_loader_common.py) checked against the oracle's own verifier, the scalar lists against what they claim
digit by digit, and the argument checks of the probes bn254_dbg_g16_loader / bn254_dbg_g16_loader_keys, which answer before any device is looked at.  No GPU."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g16_loader_common as V  # noqa: E402

SEED = 0x61D00
BAD_ARG = -1


def _g2_neg(q):
    return q[:64] + V.be((V.P - int.from_bytes(q[64:96], "big")) % V.P) + V.be((V.P - int.from_bytes(q[96:128], "big")) % V.P)


@pytest.fixture(scope="module")
def classes(pkg, O):
    return V.make_classes(pkg, O, SEED + 2, 2)


def test_scalar_lists_hold_what_they_claim():
    """Digit by digit: every 13-bit window, every comb column and every byte window takes 0 and its maximum, next to a zero and next to a non-zero digit; the top
    window takes 1, 96 and 511; tooth 12 is set where it exists; the general values are there."""
    xs = V.all_scalars()
    assert len(xs) == len(set(xs)) and set(V.general_scalars()) <= set(xs)
    for x in (0, 1, 2, V.R - 1, V.R, V.R + 1, 2 * V.R, V.P, 2 ** 255, 2 ** 254 - 1, 2 ** 256 - 1):
        assert x in xs
    fw = [V.fw_digits(x) for x in V.fw_scalars()]
    assert all(sum(d << (13 * w) for w, d in enumerate(ds)) == x for ds, x in zip(fw, V.fw_scalars()))
    assert V.fw_digits(2 ** 247 - 1) == [8191] * 19 + [0] and V.fw_digits(V.R)[19] == 96 and V.fw_digits(2 ** 256 - 1)[19] == 511 == 2 ** V.FW_TOP_BITS - 1
    for w in range(20):
        top = 511 if w == 19 else 8191
        assert {ds[w] for ds in fw} >= {0, 1, top}, w
        lone = [ds for ds in fw if ds[w] in (1, top) and sum(1 for d in ds if d) == 1]              # the digit alone: zeros before and after it
        assert {ds[w] for ds in lone} == {1, top}, w
    assert {V.fw_digits(x)[19] for x in V.fw_scalars()} >= {1, 96, 511}
    even, odd = fw[-2], fw[-1]
    assert even == [8191 if w % 2 == 0 else 0 for w in range(20)] and odd == [0 if w % 2 == 0 else (511 if w == 19 else 8191) for w in range(20)]
    comb = [V.comb_digits(x) for x in V.comb_scalars()]
    for c in range(20):
        full = 8191 if c < 16 else 4095                                                              # tooth 12 is bit 240 + c: it exists for c < 16
        assert {ds[c] for ds in comb} >= {0, 1, full}, c
        assert [ds for ds in comb if ds[c] == full and sum(1 for d in ds if d) == 1], c
        if c < 16:
            assert [ds for ds in comb if ds[c] == 1 << 12 and sum(1 for d in ds if d) == 1], c
    assert all(d < (8192 if c < 16 else 4096) for x in xs for c, d in enumerate(V.comb_digits(x)))
    assert V.comb_digits(2 ** 256 - 1) == [8191] * 16 + [4095] * 4
    by = [V.byte_digits(x) for x in V.byte_scalars()]
    for w in range(32):
        assert {ds[w] for ds in by} >= {0, 1, 255}, w
        assert {ds[w] for ds in by if ds[w] and sum(1 for d in ds if d) == 1} == {1, 255}, w
    assert by[-2] == [255, 0] * 16 and by[-1] == [0, 255] * 16


# width -> (positions, every n-th row through the verifier, every m-th of those through the pairing identity).  Widths 1 .. 33: every row of every position the GPU
# tests use (width 33: every second row).  Width 256: the GPU tests' positions, every third row (a row costs the oracle 256 multiplications); widths 32 and 241 share the builder and are not run.
TIED = {1: (None, 1, 1), 2: (None, 1, 1), 8: (None, 1, 9), 16: (None, 1, 9), 17: (None, 1, 9), 33: (None, 2, 9), 256: ([0, 15, 16, 128, 143, 240, 255], 3, 7)}


@pytest.mark.parametrize("width", sorted(TIED))
def test_rows_agree_with_the_oracle_verifier(pkg, O, classes, width):
    """For the non-degenerate rows (TIED) the generator makes a valid proof for the row's scalars and the oracle's verifier accepts it; and the row's expected L satisfies
    the verifier's own equation e(A, B) = e(alpha, beta) e(L, gamma) e(C, delta) for that proof -- which ties the builder's L to the verifier's definition of it."""
    vk_c, cl, gen = classes
    scalars = V.all_scalars()
    positions, step, pair_step = TIED[width]
    positions = list(range(width)) if positions is None else positions
    O.set_threads(8)
    vk = V.key_bytes(pkg, SEED + width, width)
    ctx = V.KeyCtx(O, vk, SEED + width)
    rows = [r for r in V.build_rows(ctx, cl, positions, scalars, zero_bg=width > 16) if r.tag[0] == "scalar"]
    assert len(rows) == len(positions) * len(scalars)
    rows = rows[::step]
    raw = b"".join(r.inputs() for r in rows)
    vk2, proofs = pkg.synth_groth16_for_inputs(SEED + width, width, raw, threads=8)
    assert vk2 == vk
    assert O.groth16_verify_many(proofs, 256, vk, raw, width, len(rows), O.MODE_GNARK) == bytes([O.ACCEPT]) * len(rows)
    dec2 = lambda b: O.decompress_g2(b, O.MODE_GNARK)[1]
    target = O.pairing(O.decompress_g1(vk[0:32])[1], dec2(vk[64:128]))
    ng, nd = _g2_neg(dec2(vk[128:192])), _g2_neg(dec2(vk[224:288]))
    for i, r in list(enumerate(rows))[::pair_step]:
        pr = proofs[256 * i:256 * i + 256]
        if width <= 33:
            assert r.L == ctx.L_of(r.xs)                                    # the background arithmetic against the plain sum
        g1 = pr[0:64] + pr[192:256] + (r.L or b"")
        g2 = pr[64:192] + nd + (ng if r.L else b"")
        assert O.pairing(g1, g2) == target, (width, r.tag)


def test_class_records_and_their_status_bytes(pkg, O, classes):
    """The class records get the byte the stage must leave: the oracle's status where A or B decides, PENDING with the deferred status of C otherwise -- and the
    oracle's verdict on the whole record agrees with that reading (a decided record: the same status; a deferred C: the status once B passed)."""
    vk, cl, gen = classes
    st = {name: cl.status(rec) for name, rec in cl.records}
    assert st["valid"] == V.PENDING and st["A = (0, 0)"] == O.ERR_NOT_ON_CURVE and st["A.x = p"] == O.ERR_NOT_MEMBER and st["A.y = p - 1"] == O.ERR_NOT_ON_CURVE
    assert st["B.x.c1 >= p"] == O.ERR_NOT_MEMBER and st["B off the twist"] == O.ERR_NOT_ON_CURVE and st["B outside G2"] == V.PENDING
    assert st["C.x >= p"] == V.PENDING | O.ERR_NOT_MEMBER == st["C.y >= p"] and st["C off the curve"] == V.PENDING | O.ERR_NOT_ON_CURVE
    assert st["A.x >= p and C off the curve"] == O.ERR_NOT_MEMBER and st["B off the twist and C off the curve"] == O.ERR_NOT_ON_CURVE
    assert st["B outside G2 and C off the curve"] == V.PENDING | O.ERR_NOT_ON_CURVE and st["B outside G2 and C.x >= p"] == V.PENDING | O.ERR_NOT_MEMBER
    for name, rec in cl.records:
        full = cl._verdict(rec)
        if not V.pending(st[name]):
            assert full == st[name], name
        elif "B outside G2" in name:
            assert full == O.ERR_NOT_IN_SUBGROUP, name
        else:
            assert full == (st[name] & 0x3f or O.ACCEPT), name
    # the generator's own failure classes: decided by the loader exactly where the oracle's status is a member / curve error of A or B
    for rec, xs, exp in gen:
        s = cl.status(rec)
        assert V.pending(s) == (exp in (O.ACCEPT, O.REJECT, O.ERR_NOT_IN_SUBGROUP)) or (s & 0x3f) == exp, exp


def test_degenerate_keys_round_trip(pkg, O):
    """A K point spliced into the key bytes comes back from the oracle's decoder, the others stay; L of the cancelling rows is the identity."""
    vk = V.key_bytes(pkg, SEED + 2, 2)
    k = V.key_points(O, vk)
    vk2 = V.splice_k(O, vk, {1: V.g1_neg(k[0])})
    k2 = V.key_points(O, vk2)
    assert k2[1] == V.g1_neg(k[0]) and k2[0] == k[0] and k2[2] == k[2] and len(vk2) == len(vk)
    ctx = V.KeyCtx(O, vk2, 1)
    assert ctx.L_of([1, 0]) is None and ctx.L_of([V.R + 1, 0]) is None and ctx.L_of([1, 5]) == V.g1_mul(O, k[2], 5) and ctx.L_of([0, 0]) == k[0]
    row = V.Row([1, 0], bytes(256), None, V.PENDING, ("t",))
    V.finish([row])
    assert row.status == V.PENDING | V.LINF and row.l_bytes == V.be(0) + V.be(1)


def test_loader_probes_check_their_arguments(pkg, O):
    """Both probes refuse each bad argument with BN254_E_BAD_ARG before any device is touched (this machine has none: any other answer would name the device)."""
    L = pkg.lib()
    fn = L.bn254_dbg_g16_loader
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.POINTER(C.c_int), C.c_int]
    narrow = pkg.PreparedVk(V.key_bytes(pkg, 7, 2), pkg.VK_GNARK)
    wide = pkg.PreparedVk(V.key_bytes(pkg, 7, 17), pkg.VK_GNARK)
    pr, rows = bytes(256 * 4), bytes(32 * 17 * 4)
    st, sst, sp, pts, info = (C.c_uint8 * 4)(), (C.c_uint8 * 4)(), (C.c_uint32 * 4)(), (C.c_uint8 * 1280)(), (C.c_int * 6)()
    good = [narrow.handle, pr, 256, rows, 2, 1, 0, 0, 0, st, sst, sp, pts, info, 0]

    def bad(**kw):
        a = list(good)
        names = ["pvk", "proofs", "stride", "inputs", "n_public", "n", "flags", "form", "misalign", "st", "sst", "sp", "pts", "info", "device"]
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    cases = [bad(pvk=None), bad(proofs=None), bad(inputs=None), bad(st=None), bad(pts=None), bad(info=None), bad(n=0), bad(n=32769), bad(stride=255),
             bad(form=-1), bad(form=4), bad(misalign=-1), bad(misalign=4), bad(flags=2), bad(flags=4), bad(flags=8),
             bad(form=1, sst=None), bad(form=1, sp=None), bad(form=1, flags=1),                       # no launch compacts under the strict flag
             bad(form=2), bad(form=3),                                                                # a wide form with a narrow key
             bad(form=2, n_public=17), bad(pvk=wide.handle, form=2, n_public=16),                     # .. or with another input count than the key's
             bad(pvk=wide.handle, form=0, n_public=17), bad(pvk=wide.handle, form=1, n_public=17),    # a wide key never sums in k_g16_prepare
             bad(pvk=wide.handle, form=1, n_public=2),                                                # .. and never compacts
             bad(pvk=wide.handle, form=3, n_public=17)]                                               # reduce8 with 2 chunks
    for a in cases:
        assert fn(*a) == BAD_ARG, a[4:9]
    fk = L.bn254_dbg_g16_loader_keys
    fk.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.POINTER(C.c_size_t), C.c_int]
    arr = (C.c_void_p * 2)(narrow.handle.value, narrow.handle.value)
    warr = (C.c_void_p * 1)(wide.handle.value)
    idx = (C.c_uint32 * 4)(0, 1, 0, 1)
    oob = (C.c_uint32 * 4)(0, 2, 0, 1)
    ns = C.c_size_t(0)
    kpts, kst, ksp = (C.c_uint8 * (320 * 128))(), (C.c_uint8 * 128)(), (C.c_uint32 * 128)()
    goodk = [arr, 2, idx, pr, 256, rows, 64, 4, 0, 0, 128, ksp, kst, kpts, C.byref(ns), 0]
    namesk = ["pvks", "n_keys", "idx", "proofs", "stride", "inputs", "in_stride", "n", "flags", "misalign", "max_slots", "sp", "sst", "pts", "ns", "device"]

    def badk(**kw):
        a = list(goodk)
        for k, v in kw.items():
            a[namesk.index(k)] = v
        return a

    for a in (badk(pvks=None), badk(n_keys=0), badk(idx=None), badk(proofs=None), badk(inputs=None), badk(sp=None), badk(sst=None), badk(pts=None), badk(ns=None),
              badk(n=0), badk(n=32769), badk(stride=255), badk(in_stride=32), badk(flags=2), badk(flags=4), badk(misalign=4), badk(misalign=-1),
              badk(idx=oob), badk(max_slots=64), badk(pvks=warr, n_keys=1)):
        assert fk(*a) == BAD_ARG, a[1:11]
    # the good calls pass every check and stop at the device this machine does not have (or run, where it has one)
    import torch
    if not torch.cuda.is_available():
        assert fn(*good) not in (0, BAD_ARG) and fk(*goodk) not in (0, BAD_ARG)
    narrow.close(); wide.close()
