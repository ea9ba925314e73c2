"""Batch verification of KZG batch-opening proofs (include/bn254_verify.h: bn254_kzg_verify_folded_batch, _device, bn254_kzg_fold_reserve) without a GPU: the limit
BN254_KZG_FOLD_MAX_DIGESTS against the planner of the G1 walk, the record length, the argument checks of the entries, and through
bn254_dbg_kzg_fold_proof(device = -1) -- the HOST compile of the loader (kzg_fold_load_record: the checks, the transcript hashed from the record, the powers of gamma,
the term records), the rows of the plan, the group sums and the pairing the kernels run -- every vector of tests/kzg_fold_common.py against hashlib, Python integers and
the oracle, byte for byte: the digest, y^, the status bytes, F and -H, their weighted forms under explicit weights, the group sums and the groups' verdicts."""
import ctypes as C
import random

import pytest

import kzg_common as Z
import kzg_fold_common as F
import pairing_batch_common as V

E_BAD_ARG = -1
NO_SUCH_DEVICE = 4097
DL = F.MAIN_DATA_LEN


@pytest.fixture(scope="module")
def key(pkg, O):
    K = Z.setup(O)
    st, key = pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"])
    assert st == V.ACCEPT
    return key


def _points(r, i):
    return r["f"][64 * i:64 * i + 64], r["h"][64 * i:64 * i + 64], tuple(r["inf"][2 * i:2 * i + 2])


def _fold(r, i):
    return r["gamma"][32 * i:32 * i + 32], r["yhat"][32 * i:32 * i + 32]


def test_max_digests_is_what_the_planner_accepts(pkg):
    """every k up to the constant plans in both forms at every launch form the planner has (split rows below the lane budget, one row per term above it, joint rows
    for large passes, and whatever lane budget and joint size the environment could force); the constant + 1 does not plan in the weighted form of a small launch"""
    M = pkg.KZG_FOLD_MAX_DIGESTS
    assert M == F.MAX_DIGESTS and 8 <= M <= 14 and pkg.KZG_FOLD_MAX_DATA == F.MAX_DATA == 64
    sizes = (1, 64, 1000, 2048, 2049, 4096, 40000, 49152, 2 ** 16, 2 ** 18)
    for k in range(1, M + 1):
        for weighted in (False, True):
            for n in sizes:
                rows = pkg.dbg_kzg_fold_plan(k, weighted, n)
                assert rows is not None and 1 <= rows <= 32, (k, weighted, n)
            for budget, joint in ((64, 0), (64, 8), (1 << 30, 0), (1 << 30, 8), (65536, 2)):
                assert pkg.dbg_kzg_fold_plan(k, weighted, 64, lane_budget=budget, joint_g=joint) is not None, (k, weighted, budget, joint)
    assert pkg.dbg_kzg_fold_plan(M + 1, True, 64) is None
    assert pkg.dbg_kzg_fold_plan(M + 1, False, 64) is not None      # the exact form alone would go one further: both must plan
    assert pkg.dbg_kzg_fold_plan(1, False, 64) == 4 and pkg.dbg_kzg_fold_plan(1, True, 64) == 8      # the rows of an opening


def test_record_length(pkg):
    assert pkg.kzg_fold_len(1, 0) == pkg.KZG_OPENING_LEN == 192
    for k in (1, 2, 13):
        for dl in (0, 5, 64):
            assert pkg.kzg_fold_len(k, dl) == 64 * k + 64 + 32 + 32 * k + dl == F.rec_len(k, dl)


@pytest.mark.parametrize("k", F.KS)
def test_vectors_hold_every_class(O, k):
    K, main, extras = F.vectors(O, k)
    names = {v.name for v in main}
    want = ["valid0", "value0_plus_one", "one_digest_identity", "h_identity", "h_identity_wrong", "z_is_tau", "z_zero", "z_ge_r", "y_last_ge_r", "d0_ge_p", "d0_off_curve",
            "h_ge_p", "h_off_curve", "order_digest_curve_before_h_ge_p", "strict_beats_both"]
    if k > 1:
        want += ["value_last_plus_one", "digests_swapped", "data_byte_flipped", "forgery_if_gamma_were_one", "all_digests_identity", "d0_identity", "dlast_ge_p", "dlast_off_curve"]
    for c in want:
        assert c in names, c
    assert {F.status(K, v) for v in main} == {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE}
    assert len(main) + sum(len(f) for _, f in extras) <= 64
    assert {(37 + 96 * k + dl) % 64 for dl, _ in extras} >= {55, 56, 63, 0} and {0, 64} <= {dl for dl, _ in extras}
    # the oracle decides: its pairing product is 1 for the valid record and not for the invalid one
    for name in ("valid0", "value0_plus_one"):
        assert F.oracle_agrees(O, K, next(v for v in main if v.name == name)), name


@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("k", F.KS)
def test_host_compile_against_python(pkg, O, key, k, strict):
    """all vectors of the main family in one probe call at a padded stride that is no multiple of 4, then packed: gamma's digest is hashlib's, y^ the integers', the
    status bytes the definition's, F and -H the oracle's; a decided record leaves zero bytes"""
    K, main, _ = F.vectors(O, k)
    flags = pkg.FLAG_STRICT_SCALARS if strict else 0
    stride = F.rec_len(k, DL) + 6
    buf, mem = F.batch(main, len(main), stride)
    r = pkg.dbg_kzg_fold_proof(key, buf, k, DL, n=len(mem), stride=stride, flags=flags, device=-1)
    want, fold = F.expected_points(O, K, mem, strict), F.expected_fold(K, mem, strict)
    for i, v in enumerate(mem):
        assert r["status"][i] == F.status(K, v, strict), (v.name, r["status"][i])
        assert _fold(r, i) == fold[i], v.name
        assert _points(r, i) == want[i], v.name
    if strict:
        assert all(r["status"][i] == V.NOT_MEMBER for i, v in enumerate(mem) if v.strict_err is not None)
    buf2, _ = F.batch(main, len(main))
    r2 = pkg.dbg_kzg_fold_proof(key, buf2, k, DL, flags=flags, device=-1)
    assert all(r2[name] == r[name] for name in ("gamma", "yhat", "f", "h", "inf", "status"))


@pytest.mark.parametrize("k", F.KS)
def test_host_compile_data_lengths_at_the_padding_edges(pkg, O, key, k):
    K, _, extras = F.vectors(O, k)
    for dl, fam in extras:
        buf, mem = F.batch(fam, len(fam))
        r = pkg.dbg_kzg_fold_proof(key, buf, k, dl, device=-1)
        fold, want = F.expected_fold(K, mem), F.expected_points(O, K, mem)
        assert r["status"] == bytes(F.status(K, v) for v in mem) == bytes([V.ACCEPT, V.REJECT]), (k, dl)
        assert all(_fold(r, i) == fold[i] and _points(r, i) == want[i] for i in range(len(mem))), (k, dl)


def _weights(rng, n):
    return ([1, 3, 2 ** 127 + 1, 2 ** 128 - 1] + [rng.randrange(2 ** 128) | 1 for _ in range(n)])[:n]


@pytest.mark.parametrize("k", F.KS)
def test_host_compile_weighted_points(pkg, O, key, k):
    """explicit weights 1, 3, 2^127 + 1, 2^128 - 1 and random odd ones: F' = r F and H' = -r H from the oracle, the group sums, and the status bytes the weighted path
    gives under these weights; gamma and y^ do not depend on the weight"""
    K, main, _ = F.vectors(O, k)
    buf, mem = F.batch(main, len(main))
    ws = _weights(random.Random(0x77 + k), len(mem))
    r = pkg.dbg_kzg_fold_proof(key, buf, k, DL, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    want, fold = F.expected_points(O, K, mem, weights=ws), F.expected_fold(K, mem)
    for i, v in enumerate(mem):
        assert _points(r, i) == want[i] and _fold(r, i) == fold[i], (v.name, ws[i])
    st, groups, failed = F.expected_rlc(O, K, mem, ws)
    assert r["status"] == st == bytes(F.status(K, v) for v in mem) and failed == 1
    assert [(a, b, tuple(c), d) for a, b, c, d in r["groups"]] == groups


@pytest.mark.parametrize("k", (1, 3, 13))
@pytest.mark.parametrize("n", (64, 65, 129))
def test_host_compile_group_sums(pkg, O, key, n, k):
    """groups of 64 with decided records and identities inside, a partial last group: the sums of the weighted points of the pending records and each group's verdict;
    a group of valid records alone passes, and null weights are all 1"""
    K, main, _ = F.vectors(O, k)
    valid = [v for v in main if F.status(K, v) == V.ACCEPT]
    errs = [v for v in main if v.err is not None]
    mem = [main[i % len(main)] for i in range(64)]
    mem += [(errs[i % len(errs)] if i % 9 == 4 else valid[i % len(valid)]) for i in range(64)]
    mem += [next(v for v in main if v.name == "value0_plus_one")]
    mem = mem[:n]
    buf = b"".join(v.rec for v in mem)
    ws = _weights(random.Random(n + k), n)
    r = pkg.dbg_kzg_fold_proof(key, buf, k, DL, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    st, groups, failed = F.expected_rlc(O, K, mem, ws)
    assert [(a, b, tuple(c), d) for a, b, c, d in r["groups"]] == groups
    assert r["status"] == st == bytes(F.status(K, v) for v in mem)
    assert [g[3] for g in groups] == [V.REJECT, V.ACCEPT, V.REJECT][:len(groups)] and failed == (2 if n > 128 else 1)
    r1 = pkg.dbg_kzg_fold_proof(key, buf, k, DL, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    st1, groups1, _ = F.expected_rlc(O, K, mem, [1] * n)
    assert [(a, b, tuple(c), d) for a, b, c, d in r1["groups"]] == groups1 and r1["status"] == st1


@pytest.mark.parametrize("k", (1, 3))
def test_cancelling_pairs_pass_under_unit_weights_and_fail_under_drawn_ones(pkg, O, key, k):
    K, main, _ = F.vectors(O, k)
    va, vb = F.forgery_pair(O, K, random.Random(0xF0 + k), k)
    valid = [v for v in main if F.status(K, v) == V.ACCEPT]
    mem = [valid[i % len(valid)] for i in range(20)]
    mem[3], mem[11] = va, vb
    buf = b"".join(v.rec for v in mem)
    r = pkg.dbg_kzg_fold_proof(key, buf, k, DL, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    assert r["groups"][0][3] == V.ACCEPT and r["status"] == bytes([V.ACCEPT] * 20)
    ws = _weights(random.Random(1), 20)
    r = pkg.dbg_kzg_fold_proof(key, buf, k, DL, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    assert r["groups"][0][3] == V.REJECT and r["status"][3] == r["status"][11] == V.REJECT and r["status"].count(V.ACCEPT) == 18
    assert pkg.dbg_kzg_fold_proof(key, buf, k, DL, device=-1)["status"] == r["status"]


def test_one_digest_without_data_is_an_opening(pkg, O, key):
    """k = 1, data_len = 0: the bytes of the host compile of the existing entry on the same records, exact and weighted"""
    K, vecs = Z.vectors(O)
    for stride in (192, 199):
        buf, mem = Z.batch(vecs, len(vecs), stride)
        for flags in (0, pkg.FLAG_STRICT_SCALARS):
            a = pkg.dbg_kzg_fold(key, buf, n=len(mem), stride=stride, flags=flags, device=-1)
            b = pkg.dbg_kzg_fold_proof(key, buf, 1, 0, n=len(mem), stride=stride, flags=flags, device=-1)
            assert all(a[name] == b[name] for name in ("f", "h", "inf", "status"))
            for i, v in enumerate(mem):      # y^ of one value is the value mod r
                assert b["yhat"][32 * i:32 * i + 32] == (V.be(v.y % V.R) if a["status"][i] in (V.ACCEPT, V.REJECT) else bytes(32))
        ws = _weights(random.Random(5), len(mem))
        a = pkg.dbg_kzg_fold(key, buf, n=len(mem), stride=stride, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
        b = pkg.dbg_kzg_fold_proof(key, buf, 1, 0, n=len(mem), stride=stride, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
        assert all(a[name] == b[name] for name in ("f", "h", "inf", "status", "groups"))


def test_argument_errors_touch_nothing(pkg, O, key):
    K, main, _ = F.vectors(O, 2)
    L = pkg.lib()
    L.bn254_last_error.restype = C.c_char_p
    L.bn254_kzg_verify_folded_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    L.bn254_kzg_verify_folded_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    L.bn254_dbg_kzg_fold_proof.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.bn254_kzg_fold_reserve.argtypes = [C.c_size_t, C.c_size_t, C.c_int]
    st = (C.c_uint8 * 4)(*([0xEE] * 4))
    stp = C.cast(st, C.c_void_p)
    scratch = (C.c_uint8 * 1024)()
    sp = C.cast(scratch, C.c_void_p)
    item = main[0].rec * 2
    rl = F.rec_len(2, DL)
    kbuf = C.create_string_buffer(key, len(key))
    kp, ip = C.cast(kbuf, C.c_void_p), C.cast(C.create_string_buffer(item, len(item)), C.c_void_p)
    M = pkg.KZG_FOLD_MAX_DIGESTS

    def untouched():
        return bytes(st) == b"\xee" * 4

    host = lambda k_, o, s, n, kd, dl, status, flags: L.bn254_kzg_verify_folded_batch(k_, o, s, n, kd, dl, status, NO_SUCH_DEVICE, flags)
    probe = lambda k_, o, s, n, kd, dl, status, flags: L.bn254_dbg_kzg_fold_proof(k_, o, s, n, kd, dl, None, flags, sp, sp, sp, sp, status, None, NO_SUCH_DEVICE, 0)
    probe_host = lambda k_, o, s, n, kd, dl, status, flags: L.bn254_dbg_kzg_fold_proof(k_, o, s, n, kd, dl, None, flags, sp, sp, sp, sp, status, None, -1, 0)
    dev = lambda k_, o, s, n, kd, dl, status, flags: L.bn254_kzg_verify_folded_batch_device(kp if k_ is not None else None, ip if o is not None else None, s, n, kd, dl, status,
                                                                                            NO_SUCH_DEVICE, None, flags)
    bad_key = bytearray(key); bad_key[0] ^= 1
    for name, call in (("host", host), ("probe", probe), ("probe_host", probe_host), ("device", dev)):
        assert call(None, item, rl, 1, 2, DL, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(key, None, rl, 1, 2, DL, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(key, item, rl, 1, 2, DL, None, 0) == E_BAD_ARG and untouched(), name
        assert call(key, item, rl - 1, 1, 2, DL, stp, 0) == E_BAD_ARG and untouched(), name                   # stride below the record length
        assert b"stride" in L.bn254_last_error(), name
        assert call(key, item, rl, 1, 2, DL + 1, stp, 0) == E_BAD_ARG and untouched(), name                   # ... of THIS data_len
        assert call(key, item, 4096, 1, 0, 0, stp, 0) == E_BAD_ARG and untouched(), name                      # k = 0
        assert call(key, item, 4096, 1, M + 1, 0, stp, 0) == E_BAD_ARG and untouched(), name
        assert b"n_digests" in L.bn254_last_error(), name
        assert call(key, item, 4096, 1, 2, pkg.KZG_FOLD_MAX_DATA + 1, stp, 0) == E_BAD_ARG and untouched(), name
        assert b"data_len" in L.bn254_last_error(), name
        assert call(key, item, 4096, 0, M + 1, 0, stp, 0) == E_BAD_ARG, name                                  # the shape is checked even for n == 0
        assert call(key, item, rl, 1, 2, DL, stp, 4) == E_BAD_ARG and call(key, item, rl, 1, 2, DL, stp, 8 | pkg.FLAG_RLC) == E_BAD_ARG and untouched(), name
        assert call(key, item, 2 ** 63, 3, 2, DL, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(key, item, rl, 0, 2, DL, stp, 0) == 0 and call(None, None, rl, 0, 2, DL, None, pkg.FLAG_RLC) == 0 and untouched(), name      # n == 0
        if name not in ("probe_host", "device"):
            assert call(bytes(bad_key), item, rl, 1, 2, DL, stp, 0) == E_BAD_ARG and untouched() and b"magic" in L.bn254_last_error(), name
        if name != "probe_host":
            rc = call(key, item, rl, 2, 2, DL, stp, pkg.FLAG_RLC | pkg.FLAG_STRICT_SCALARS)                   # past the argument checks: the device ordinal
            assert rc in (-1, -2) and untouched() and b"device" in L.bn254_last_error().lower(), name
    assert L.bn254_kzg_verify_folded_batch_device(C.c_void_p(kp.value + 2), ip, rl, 1, 2, DL, stp, NO_SUCH_DEVICE, None, 0) == E_BAD_ARG and b"aligned" in L.bn254_last_error()
    assert L.bn254_kzg_fold_reserve(10, 0, NO_SUCH_DEVICE) == E_BAD_ARG and L.bn254_kzg_fold_reserve(10, M + 1, NO_SUCH_DEVICE) == E_BAD_ARG
    assert L.bn254_kzg_fold_reserve(10, 2, NO_SUCH_DEVICE) in (-1, -2) and b"device" in L.bn254_last_error().lower()
    # the probe's own rules, as bn254_dbg_kzg_fold's
    w = bytes(32)
    assert L.bn254_dbg_kzg_fold_proof(key, item, rl, 2, 2, DL, w, 0, sp, sp, sp, sp, stp, None, -1, 0) == E_BAD_ARG and untouched()
    assert L.bn254_dbg_kzg_fold_proof(key, item, rl, 2, 2, DL, None, 0, sp, sp, sp, sp, stp, sp, -1, 0) == E_BAD_ARG and untouched()
    assert L.bn254_dbg_kzg_fold_proof(key, item, rl, 2, 2, DL, None, 0, sp, sp, sp, sp, stp, None, -1, 1) == E_BAD_ARG and untouched()
    assert L.bn254_dbg_kzg_fold_proof(key, item, rl, 2, 2, DL, None, 0, None, sp, sp, sp, stp, None, -1, 0) == E_BAD_ARG and untouched()
    assert untouched()
