"""The device self-test (include/bn254_verify.h, bn254_device_selftest) without a device: its built-in vectors against the oracle, and its interface.

The known answers the library compares the kernels' output with come from tables of gen_constants.py (the statuses of the Groth16 and two-pair checks) and from the
host's compile of the arithmetic the kernels run (everything else).  Here every one of them is recomputed by the oracle from the vectors' INPUTS, so that they are
pinned to something other than the code under test, wherever the library took them from."""
import ctypes as C

import pytest

NAMES = ["fp", "fp12_lane", "fp12_coop", "pairing_lane", "g16_lane", "g16_coop", "pair2_lane", "pair2_coop", "codec", "sha256"]
E_NO_DEVICE, E_BAD_ARG = -2, -1
ONE_GT = (1).to_bytes(32, "big") + bytes(352)


@pytest.fixture(scope="module")
def lib(pkg):
    l = pkg.lib()
    l.bn254_selftest_check_name.restype = C.c_char_p
    l.bn254_last_error.restype = C.c_char_p
    return l


@pytest.fixture(scope="module")
def vectors(lib):
    """{check: (inputs, expected)} from bn254_dbg_selftest_vectors, read once"""
    out = {}
    for k in range(10):
        n_in, n_ex = C.c_size_t(), C.c_size_t()
        assert lib.bn254_dbg_selftest_vectors(k, None, C.c_size_t(0), C.byref(n_in), None, C.c_size_t(0), C.byref(n_ex)) == E_BAD_ARG      # the lengths are still written
        a, b = (C.c_uint8 * n_in.value)(), (C.c_uint8 * n_ex.value)()
        assert lib.bn254_dbg_selftest_vectors(k, a, n_in, C.byref(n_in), b, n_ex, C.byref(n_ex)) == 0
        out[k] = (bytes(a), bytes(b))
    return out


def _i(b):
    return int.from_bytes(b, "big")


def _chunks(b, n):
    return [b[i:i + n] for i in range(0, len(b), n)]


def test_fp_products_match_the_oracle(vectors, O):
    inp, exp = vectors[0]
    a, b = _chunks(inp[:2048], 32), _chunks(inp[2048:], 32)
    assert len(a) == len(b) == 64
    vals = {_i(x) for x in a} | {_i(x) for x in b}
    assert {0, 1, O.P - 1, O.P - 2} <= vals and all(v < O.P for v in vals)
    assert _chunks(exp, 32) == [O.be32(O.fp_op(2, _i(x), _i(y))) for x, y in zip(a, b)]


def _easy(O, a):
    t = O.fp12_op(0, O.fp12_op(7, a), O.fp12_op(2, a))      # conj(a) / a
    return O.fp12_op(0, O.fp12_op(4, t), t)                 # ^(p^2 + 1)


def test_fp12_lane_values_match_the_oracle(vectors, O):
    inp, exp = vectors[1]
    v = _chunks(inp, 384)
    a, b, c = v[0:2], v[2:4], v[4:6]
    want = [[O.fp12_op(0, x, y) for x, y in zip(a, b)], [O.fp12_op(1, x) for x in a], [O.fp12_op(2, x) for x in a], [O.fp12_op(6, _easy(O, x)) for x in a],
            [O.fp12_op(3, x) for x in a], [O.fp12_op(6, x) for x in c], [O.fp12_op(4, x) for x in a], [O.fp12_op(5, x) for x in a]]
    assert _chunks(exp, 384) == [x for op in want for x in op]
    # c is cyclotomic: the cyclotomic squaring and the general one agree on it
    assert all(O.fp12_op(6, x) == O.fp12_op(1, x) for x in c)


def test_fp12_coop_values_match_the_oracle(vectors, O):
    inp, exp = vectors[2]
    v = _chunks(inp, 384)
    a, b, c = v[0:6], v[6:12], v[12:18]
    sq3 = lambda x: O.fp12_op(6, O.fp12_op(6, O.fp12_op(6, x)))
    want = [[O.fp12_op(0, x, y) for x, y in zip(a, b)], [O.fp12_op(1, x) for x in a], [sq3(x) for x in c], [O.fp12_op(3, x) for x in a], [O.fp12_op(4, x) for x in a],
            [O.fp12_op(5, x) for x in a], [O.fp12_op(2, x) for x in a], [O.final_exp(x) for x in a]]
    assert _chunks(exp, 384) == [x for op in want for x in op]
    assert all(O.fp12_op(6, x) == O.fp12_op(1, x) for x in c)


def test_pairings_match_the_oracle(vectors, O):
    inp, exp = vectors[3]
    g1, g2 = _chunks(inp[:256], 64), _chunks(inp[256:], 128)
    assert g1[0] == O.g1_gen() and g2[0] == O.g2_gen()
    gt = _chunks(exp, 384)
    assert gt == [O.pairing(p, q) for p, q in zip(g1, g2)]
    assert O.fp12_op(0, gt[1], gt[2]) == ONE_GT and gt[1] != ONE_GT        # e(aG1, bG2) e(-aG1, bG2) = 1


@pytest.mark.parametrize("check", [4, 5])
def test_groth16_statuses_match_the_oracle_and_hold_every_class(vectors, O, check):
    inp, exp = vectors[check]
    vk, proofs, inputs = inp[:520], inp[520:520 + 64 * 256], inp[520 + 64 * 256:]
    assert len(inputs) == 64 * 64 and len(exp) == 64
    assert exp == O.groth16_verify_many(proofs, 256, vk, inputs, 2, 64, O.MODE_REFERENCE)
    assert set(exp) == {O.ACCEPT, O.REJECT, O.ERR_NOT_ON_CURVE, O.ERR_NOT_IN_SUBGROUP, O.ERR_NOT_MEMBER}
    # both kinds of REJECT: by a public input (the same proof verifies with the input one lower) and by C
    rejected = [i for i in range(64) if exp[i] == O.REJECT]
    by_input = []
    for i in rejected:
        row = inputs[64 * i:64 * i + 64]
        fixed = O.be32(_i(row[:32]) - 1) + row[32:]
        by_input.append(O.groth16_verify_many(proofs[256 * i:256 * i + 256], 256, vk, fixed, 2, 1, O.MODE_REFERENCE) == bytes([O.ACCEPT]))
    assert any(by_input) and not all(by_input)
    assert vectors[4] == vectors[5]


@pytest.mark.parametrize("check", [6, 7])
def test_two_pair_statuses_match_the_oracle(vectors, O, check):
    inp, exp = vectors[check]
    q0, q1, target = inp[0:128], inp[128:256], inp[256:640]
    p0, p1, flags = _chunks(inp[640:640 + 4096], 64), _chunks(inp[640 + 4096:640 + 8192], 64), inp[640 + 8192:]
    assert len(flags) == 64 and target == ONE_GT
    # the G2 points are those of the built-in key's line tables: gamma as the reference decodes it, delta negated (csrc/bn254_host.hpp::prepare_g16)
    vk = vectors[4][0][:520]
    st, g = O.decompress_g2(vk[128:192], O.MODE_REFERENCE)
    st2, d = O.decompress_g2(vk[224:288], O.MODE_REFERENCE)
    neg = lambda v: O.be32((O.P - _i(v)) % O.P)
    assert st == st2 == O.ACCEPT and q0 == g and q1 == d[:64] + neg(d[64:96]) + neg(d[96:128])
    want = []
    for i in range(64):
        g1s = (p0[i] if not flags[i] & 1 else b"") + (p1[i] if not flags[i] & 2 else b"")
        g2s = (q0 if not flags[i] & 1 else b"") + (q1 if not flags[i] & 2 else b"")
        gt = O.final_exp(O.miller_loop(g1s, g2s)) if g1s else ONE_GT
        want.append(O.ACCEPT if gt == target else O.ERR_PAIRING_FAILED)
        if flags[i] & 1:
            assert p0[i] == bytes(32) + O.be32(1)
        if flags[i] & 2:
            assert p1[i] == bytes(32) + O.be32(1)
    assert exp == bytes(want)
    assert set(exp) == {O.ACCEPT, O.ERR_PAIRING_FAILED} and any(flags)
    assert {exp[i] for i in range(64) if flags[i]} == {O.ACCEPT, O.ERR_PAIRING_FAILED}      # an identity argument on both sides of the verdict


def test_codec_records_match_the_oracle(vectors, O):
    inp, exp = vectors[8]
    recs, raw, pre = _chunks(inp, 128), _chunks(exp[:11 * 256], 256), exp[11 * 256:]
    assert len(recs) == 11 and len(pre) == 11
    for r, w, bad in zip(recs, raw, pre):
        s1, a = O.decompress_g1(r[0:32]); s2, b = O.decompress_g2(r[32:96], O.MODE_GNARK); s3, c = O.decompress_g1(r[96:128])
        ok = s1 == s2 == s3 == O.ACCEPT
        assert bad == (0 if ok else 1)
        assert w == (a + b + c if ok else b"\xff" * 256)
    proofs = vectors[4][0][520:]
    assert raw[:8] == _chunks(proofs[:8 * 256], 256)             # the first eight: the built-in proofs back
    assert list(pre) == [0] * 8 + [1, 1, 0]
    assert recs[8][0] >> 6 == 0 and recs[10][32] == 0x40 and raw[10][64:192] == O.g2_gen()


def test_sha256_rows_match_the_oracle(vectors, O):
    inp, exp = vectors[9]
    vkh = _chunks(inp[:256], 32)
    off = [int.from_bytes(x, "little") for x in _chunks(inp[256:256 + 72], 8)]
    pv_bytes = int.from_bytes(inp[328:336], "little")
    pv = inp[336:]
    assert pv_bytes == len(pv) == 1424
    assert [off[i + 1] - off[i] for i in range(7)] == [0, 55, 56, 64, 119, 120, 1000] and all(o % 4 for o in off[:8])
    rows, pre = _chunks(exp[:512], 64), exp[512:]
    for i in range(8):
        inside = off[i] <= off[i + 1] <= pv_bytes
        d = bytearray(O.sha256(pv[off[i]:off[i + 1]] if inside else b""))
        d[0] &= 0x1f                                             # SP1 clears the top three bits of the digest
        assert rows[i] == vkh[i] + bytes(d) and pre[i] == (0 if inside else 1)
    assert list(pre) == [0] * 7 + [1]


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_check_names(lib):
    names = [lib.bn254_selftest_check_name(k).decode() for k in range(10)]
    assert names == NAMES and len(set(names)) == 10 and all(names)
    assert lib.bn254_selftest_check_name(-1) == b"" and lib.bn254_selftest_check_name(10) == b""
    state = C.c_int(7)
    assert lib.bn254_dbg_selftest(0, 10, 0, None) == E_BAD_ARG and lib.bn254_device_selftest_state(64, C.byref(state), None) == E_BAD_ARG
    assert lib.bn254_device_selftest_state(0, None, None) == E_BAD_ARG


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-GPU failure mode")
def test_interface_without_a_device(lib):
    state, mask, ms = C.c_int(7), C.c_uint(7), C.c_float(7)
    assert lib.bn254_device_selftest_state(0, C.byref(state), C.byref(mask)) == 0 and state.value == -1 and mask.value == 0
    assert lib.bn254_device_selftest(0, C.byref(mask), C.byref(ms)) == E_NO_DEVICE and b"no HIP device" in lib.bn254_last_error()
    assert lib.bn254_device_selftest(0, None, None) == E_NO_DEVICE
    assert lib.bn254_dbg_selftest(0, 4, 1, None) == E_NO_DEVICE
    assert lib.bn254_device_selftest_state(0, C.byref(state), None) == 0 and state.value == -1      # nothing above touched it
