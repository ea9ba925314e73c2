"""bn254_groth16_vk_prepare_batch without a GPU (include/bn254_verify.h, "Many keys prepared in one call").

The definition of correctness is the header's: key_status[i] is the return code of bn254_groth16_vk_prepare on key i, out[i] is NULL for a key that does not load and
otherwise a handle whose host image (bn254_dbg_g16_pvk_image) equals the single-key handle's dword for dword.  Here the bodies of the new kernels (csrc/bn254_vkprep.h)
run compiled for the host, behind bn254_dbg_g16_vk_prepare_batch(device = -1): the projective line-table walk with one inversion against the host's affine walk with
an inversion per step, the decode lanes against parse_g16_vk, the fold against prepare_g16's negations.  The argument rules of the public entry are checked too; with
valid arguments and no device it answers BN254_E_NO_DEVICE (there is no CPU fallback)."""
import ctypes as C
import random

import pytest

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
OK, E_BAD_ARG, E_NO_DEVICE, E_VK = 0, -1, -2, -4
WIDTHS = (0, 1, 2, 5, 16, 17, 40)


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def be(v):
    return int(v).to_bytes(32, "big")


def _twist_point(O, rng):
    """a random point of the twist, uncompressed (as tests/test_edge_keys.py makes them): off the r-torsion with probability 1 - 1 / cofactor"""
    bt = O.fp2_op(2, O.fp2_op(3, (9, 1)), (3, 0))
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        rhs = O.fp2_op(0, O.fp2_op(2, O.fp2_op(5, x), x), bt)
        y = O.fp2_op(4, rhs)
        if y != (0, 0) and O.fp2_op(5, y) == rhs:
            return be(x[1]) + be(x[0]) + be(y[1]) + be(y[0])


def _synth_vk(pkg, seed, n_public, agree=True):
    return pkg.synth_groth16(seed, n_public, 0, invalid_every=0, agree=agree, threads=1)[0]


def _single(pkg, vk, mode):
    """(return code, PreparedVk or None) of the single-key entry"""
    h = C.c_void_p()
    rc = pkg.lib().bn254_groth16_vk_prepare(bytes(vk), len(vk), mode, C.byref(h))
    if rc != OK:
        assert not h.value
        return rc, None
    k = pkg.PreparedVk.__new__(pkg.PreparedVk)
    k._h = h
    k.n_public = pkg.lib().bn254_groth16_vk_num_public(h)
    return rc, k


def check_list(pkg, vks, mode, device=-1, want_loaded=None):
    """the whole definition for one list: statuses, NULLs and images against the single-key entry.  Returns the statuses."""
    if device == -1:
        keys, status, _ = pkg.dbg_prepare_vks(vks, mode, -1)
    else:
        keys, status = pkg.prepare_vks(vks, mode, device, with_status=True)
    assert len(keys) == len(status) == len(vks)
    for i, vk in enumerate(vks):
        rc, ref = _single(pkg, vk, mode)
        assert status[i] == rc, (i, status[i], rc)
        assert (keys[i] is None) == (ref is None), i
        if ref is not None:
            assert keys[i].n_public == ref.n_public
            assert pkg.dbg_pvk_image(keys[i]) == pkg.dbg_pvk_image(ref), "image of key %d differs (mode %d)" % (i, mode)
            ref.close()
    if want_loaded is not None:
        assert [s == OK for s in status] == want_loaded, status
    for k in keys:
        if k is not None:
            k.close()
    return status


@pytest.fixture(scope="module")
def good_keys(pkg):
    """the generator's keys at every width, mode-agreeing, and at three widths keys whose two G2 root orders differ (agree = 0)"""
    return [_synth_vk(pkg, 0x5B0000 + w, w) for w in WIDTHS] + [_synth_vk(pkg, 0x5B1000 + w, w, agree=False) for w in (1, 2, 17)]


def _without_k(vk1):
    """the zero-input key's bytes without its K point (nK = 0)"""
    return vk1[:288] + (0).to_bytes(4, "big") + vk1[292 + 32:]


@pytest.mark.parametrize("mode", [0, 1])
def test_host_compile_of_the_kernels_matches_the_single_key_path(pkg, O, good_keys, mode):
    rng = random.Random(0xB47C)
    vks = list(good_keys)
    vks.append(_without_k(good_keys[0]))                                      # a key without K points: the generator as k0, n_k = 0
    inf = bytearray(good_keys[2]); inf[128:192] = bytes([0x40]) + bytes(63)   # gamma with the infinity flag: decodes to the G2 generator
    vks.append(bytes(inf))
    for off in (64, 128, 224):                                                # beta, gamma, delta off the r-torsion: the loader does not check, the walk still has its lines
        q = _twist_point(O, rng)
        assert O.g2_subgroup_check(q) == 0
        k = bytearray(good_keys[2]); k[off:off + 64] = O.compress_g2(q)
        vks.append(bytes(k))
    h = 2 * P - R
    while True:                                                               # ... and of the small order 10069
        q = O.g2_mul(_twist_point(O, rng), R)
        q = O.g2_mul(q, h // 10069) if q != bytes(128) else q
        if q != bytes(128):
            break
    k = bytearray(good_keys[1]); k[224:288] = O.compress_g2(q)
    vks.append(bytes(k))
    check_list(pkg, vks, mode, want_loaded=[True] * len(vks))


def _no_root_g1(pkg, vk, off):
    """the key with the G1 point at `off` replaced by an x for which x^3 + 3 has no root (flag 0b10)"""
    x = 5
    while pow((x ** 3 + 3) % P, (P - 1) // 2, P) == 1:
        x += 1
    b = bytearray(vk); b[off:off + 32] = be(x); b[off] |= 0x80
    return bytes(b)


def _no_root_g2(pkg, vk, off, mode):
    """... and a G2 point at `off` whose x has no y on the twist: found against the single-key entry, which is the definition"""
    for x0 in range(1, 64):
        b = bytearray(vk); b[off:off + 64] = be(7) + be(x0); b[off] |= 0x80
        if _single(pkg, bytes(b), mode)[0] == E_VK:
            return bytes(b)
    raise AssertionError("no x without a root among 63 candidates")


def bad_keys(pkg, vk, n_public, mode):
    """[(label, bytes)] of keys made from the good key vk (n_public inputs) that must not load"""
    nk = n_public + 1
    k_end = 292 + 32 * nk
    out = []
    for cut in sorted({0, 31, 32, 64, 128, 192, 224, 288, 291, 292, 292 + 31, k_end - 1, k_end, k_end + 3, k_end + 4, k_end + 4 + 63, k_end + 4 + 64, len(vk) - 1}):
        out.append(("truncated at %d" % cut, vk[:cut]))
    points = [0, 32, 64, 128, 192, 224] + [292 + 32 * i for i in range(nk)] + [k_end + 4, k_end + 4 + 64]
    for off in points:
        b = bytearray(vk); b[off] &= 0x3f
        out.append(("flag 00 at %d" % off, bytes(b)))
    out.append(("G1 x without a root (alpha)", _no_root_g1(pkg, vk, 0)))
    out.append(("G1 x without a root (last K)", _no_root_g1(pkg, vk, 292 + 32 * (nk - 1))))
    out.append(("G2 x without a root (gamma)", _no_root_g2(pkg, vk, 128, mode)))
    out.append(("G2 x without a root (commitment key)", _no_root_g2(pkg, vk, k_end + 4 + 64, mode)))
    b = bytearray(vk); b[288:292] = (nk + 5).to_bytes(4, "big")
    out.append(("K count larger than the buffer", bytes(b)))
    b = bytearray(vk); b[288:292] = (0xFFFFFFFF).to_bytes(4, "big")
    out.append(("K count 2^32 - 1", bytes(b)))
    b = bytearray(vk); b[k_end:k_end + 4] = (0xFFFFFFFF).to_bytes(4, "big")
    out.append(("2^32 - 1 commitment-index vectors", bytes(b)))
    out.append(("one commitment-index vector of 2^32 - 1 entries", vk[:k_end] + (1).to_bytes(4, "big") + (0xFFFFFFFF).to_bytes(4, "big") + vk[k_end + 4:]))
    out.append(("missing trailer", vk[:k_end + 4]))
    out.append(("commitment indices that eat the trailer", vk[:k_end] + (1).to_bytes(4, "big") + (16).to_bytes(4, "big") + vk[k_end + 4:]))
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_bad_keys_inside_a_good_list(pkg, good_keys, mode):
    """every bad key between good neighbours: its status is the single-key return code (BN254_E_VK), its handle NULL, and every good key of the list keeps the image
    it has alone"""
    vk2 = good_keys[2]
    bad = bad_keys(pkg, vk2, 2, mode)
    for label, b in bad:
        assert _single(pkg, b, mode)[0] == E_VK, label                       # (the cases are bad by the definition, not by this test's opinion)
    vks, loaded = [], []
    for i, (label, b) in enumerate(bad):
        vks += [good_keys[i % len(good_keys)], b]
        loaded += [True, False]
    vks.append(vk2); loaded.append(True)
    check_list(pkg, vks, mode, want_loaded=loaded)
    # a list of bad keys only, and bad keys at both ends
    check_list(pkg, [b for _, b in bad[:6]], mode, want_loaded=[False] * 6)
    check_list(pkg, [bad[0][1], vk2, bad[-1][1]], mode, want_loaded=[False, True, False])


def test_argument_errors_and_the_empty_list(pkg, good_keys):
    L = pkg.lib()
    fn = L.bn254_groth16_vk_prepare_batch
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    vks = [good_keys[2], good_keys[0]]
    ptrs = (C.c_char_p * 2)(*vks)
    lens = (C.c_size_t * 2)(*[len(v) for v in vks])
    out = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
    st = (C.c_int * 2)(77, 77)
    assert fn(None, None, 0, 0, 0, None, None) == OK                          # n_keys = 0: nothing is looked at
    assert fn(ptrs, lens, 0, 0, 0, out, st) == OK and list(st) == [77, 77]
    for args in ((None, lens, out, st), (ptrs, None, out, st), (ptrs, lens, None, st), (ptrs, lens, out, None)):
        assert fn(args[0], args[1], 2, 0, 0, args[2], args[3]) == E_BAD_ARG
    assert fn(ptrs, lens, 2, 2, 0, out, st) == E_BAD_ARG                      # mode > 1
    holes = (C.c_char_p * 2)(vks[0], None)
    assert fn(holes, lens, 2, 0, 0, out, st) == E_BAD_ARG                     # a null key in the list
    rc = fn(ptrs, lens, 2, 1, 0, out, st)
    if _have_gpu():
        assert rc == OK and list(st) == [OK, OK] and out[0] and out[1]
        for h in out:
            L.bn254_groth16_vk_free(h)
    else:
        assert rc == E_NO_DEVICE and not out[0] and not out[1]               # no CPU fallback; on a negative return every out[i] is NULL
    # the probe takes the same arguments and checks them the same way
    pr = L.bn254_dbg_g16_vk_prepare_batch
    pr.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert pr(ptrs, lens, 2, 2, -1, out, st, None) == E_BAD_ARG
    assert pr(holes, lens, 2, 0, -1, out, st, None) == E_BAD_ARG
    assert pr(ptrs, lens, 2, 0, -2, out, st, None) == E_BAD_ARG
    assert pr(None, None, 0, 0, -1, None, None, None) == OK
    # the image probe: its length first, then a buffer that is too small
    k = pkg.PreparedVk(vks[0])
    im = pkg.dbg_pvk_image(k)
    ln = C.c_size_t(0)
    ip = L.bn254_dbg_g16_pvk_image
    ip.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    small = (C.c_uint8 * 16)()
    assert ip(k.handle, small, 16, C.byref(ln)) == E_BAD_ARG and ln.value == len(im)
    assert ip(None, small, 16, C.byref(ln)) == E_BAD_ARG
    assert len(im) == 4 * (3 + 5 + 18 + 2 * 88 * 54 + 108 + 2 * 18 + 18 + 18 + 36)    # a 2-input key: k0, two line tables, the target, two K points, alpha, k0, b
    k.close()


def test_more_keys_than_a_pass_and_independent_handles(pkg, good_keys):
    """handles are independent: freeing them in any order, and keeping one while the others go, leaves it usable (its image still reads the same)"""
    vks = [good_keys[i % len(good_keys)] for i in range(9)]
    keys, status, _ = pkg.dbg_prepare_vks(vks, 0, -1)
    assert status == [OK] * 9
    want = pkg.dbg_pvk_image(keys[4])
    for i in (8, 0, 3, 7, 1, 6, 2, 5):
        keys[i].close()
    assert pkg.dbg_pvk_image(keys[4]) == want
    keys[4].close()
