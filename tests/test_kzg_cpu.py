"""Batch verification of KZG openings (include/bn254_verify.h: bn254_kzg_key_prepare, bn254_kzg_verify_batch, _device, the knob) without a GPU: the key record, the
argument checks of both entries, the knob, and through bn254_dbg_kzg_fold(device = -1) -- the HOST compile of the loader (kzg_load_opening), the rows of the G1
walk's plan, the group sums and the mixed Miller run the kernels run -- every vector class of tests/kzg_common.py against Python integers and the oracle, byte for
byte: status bytes, the points F_i and -H_i, their weighted forms under explicit weights, the group sums and the groups' verdicts."""
import ctypes as C
import random
import struct

import pytest

import kzg_common as Z
import pairing_batch_common as V

E_BAD_ARG = -1
NO_SUCH_DEVICE = 4097
MAGIC, VERSION = 0x59474B42, 1
HDR, G1_DIGITS = 16, 72


@pytest.fixture(scope="module")
def kzg(pkg, O):
    K, vecs = Z.vectors(O)
    st, key = pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"])
    assert st == V.ACCEPT and len(key) == pkg.KZG_KEY_LEN
    return K, vecs, key


def _points(r, i):
    return r["f"][64 * i:64 * i + 64], r["h"][64 * i:64 * i + 64], tuple(r["inf"][2 * i:2 * i + 2])


def test_key_len_is_the_layout(pkg):
    assert pkg.KZG_KEY_LEN == HDR + G1_DIGITS + 2 * pkg.G2_PREPARED_LEN == 38424 and pkg.KZG_OPENING_LEN == 192 == 6 * 32


def test_key_prepare(pkg, O):
    K = Z.setup(O)
    st, key = pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"])
    assert st == V.ACCEPT
    assert struct.unpack_from("<4I", key) == (MAGIC, VERSION, 0, 0)
    # the two G2 parts are byte for byte what g2_prepare writes
    for j, q in enumerate((K["g2"], K["tau_g2"])):
        s, rec = pkg.g2_prepare(q)
        assert s == V.ACCEPT and key[HDR + G1_DIGITS + j * pkg.G2_PREPARED_LEN:HDR + G1_DIGITS + (j + 1) * pkg.G2_PREPARED_LEN] == rec
    assert pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"]) == (st, key)            # a pure function of the bytes
    # identities are accepted and flagged: g1 in the key's flag word, the G2 points in their records'
    st0, key0 = pkg.kzg_key_prepare(bytes(64), bytes(128), K["tau_g2"])
    assert st0 == V.ACCEPT and struct.unpack_from("<4I", key0) == (MAGIC, VERSION, 1, 0) and not any(key0[HDR:HDR + G1_DIGITS])
    assert struct.unpack_from("<4I", key0, HDR + G1_DIGITS)[2] == 1 and struct.unpack_from("<4I", key0, HDR + G1_DIGITS + pkg.G2_PREPARED_LEN)[2] == 0
    assert struct.unpack_from("<4I", pkg.kzg_key_prepare(K["g1"], K["g2"], bytes(128))[1], HDR + G1_DIGITS + pkg.G2_PREPARED_LEN)[2] == 1
    # every status of the key, for each of the three points, the first failure deciding; out untouched, the return code OK
    L = pkg.lib()
    L.bn254_kzg_key_prepare.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
    rng = random.Random(0x6B)
    g1_ge_p, g1_off = V.be(V.P + 1) + K["g1"][32:], V.add_to_field(K["g1"], 32, 1)
    g2_ge_p, g2_off, g2_far = K["g2"][:64] + V.be(V.P + 2) + K["g2"][96:], V.add_to_field(K["g2"], 96, 1), V.outside_g2(O, rng)
    cases = [((g1_ge_p, K["g2"], K["tau_g2"]), V.NOT_MEMBER), ((g1_off, K["g2"], K["tau_g2"]), V.NOT_ON_CURVE)]
    for pos in (1, 2):
        for bad, want in ((g2_ge_p, V.NOT_MEMBER), (g2_off, V.NOT_ON_CURVE), (g2_far, V.NOT_IN_SUBGROUP)):
            pts = [K["g1"], K["g2"], K["tau_g2"]]
            pts[pos] = bad
            cases.append((tuple(pts), want))
    cases.append(((g1_off, g2_ge_p, g2_far), V.NOT_ON_CURVE))       # the first failure over g1, g2, tau_g2
    cases.append(((K["g1"], g2_far, g2_ge_p), V.NOT_IN_SUBGROUP))
    for pts, want in cases:
        out = (C.c_uint8 * pkg.KZG_KEY_LEN)(*([0xEE] * pkg.KZG_KEY_LEN)); s = C.c_uint8(0xEE)
        assert L.bn254_kzg_key_prepare(pts[0], pts[1], pts[2], out, C.byref(s)) == 0
        assert s.value == want and bytes(out) == b"\xee" * pkg.KZG_KEY_LEN, want
        assert pkg.kzg_key_prepare(*pts) == (want, None)
    out = (C.c_uint8 * pkg.KZG_KEY_LEN)(); s = C.c_uint8(0xEE)
    for args in ((None, K["g2"], K["tau_g2"], out, C.byref(s)), (K["g1"], None, K["tau_g2"], out, C.byref(s)), (K["g1"], K["g2"], None, out, C.byref(s)),
                 (K["g1"], K["g2"], K["tau_g2"], None, C.byref(s)), (K["g1"], K["g2"], K["tau_g2"], out, None)):
        assert L.bn254_kzg_key_prepare(*args) == E_BAD_ARG
    assert s.value == 0xEE


def test_vectors_hold_every_class(O):
    K, vecs = Z.vectors(O)
    assert len(vecs) <= 64
    names = {v.name for v in vecs}
    for c in ("valid0", "value_plus_one", "wrong_quotient", "z_ge_r", "y_ge_r", "both_ge_r", "y_zero", "z_zero", "z_is_tau", "c_identity", "h_identity", "h_identity_wrong",
              "f_identity", "c_ge_p", "h_ge_p", "c_off_curve", "h_off_curve", "order_c_curve_before_h_ge_p", "order_c_ge_p_before_h_curve", "strict_beats_curve"):
        assert c in names, c
    assert Z.status_classes(K, vecs) == {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE}
    assert K["s"] != 1


@pytest.mark.parametrize("strict", (False, True))
def test_host_compile_against_the_oracle(pkg, O, kzg, strict):
    """all vectors in one probe call at a padded stride that is no multiple of 4: the status bytes are the definition's, the points of every opening that reaches the
    pairing are the oracle's F_i = C_i - y_i g1 + z_i H_i and -H_i, a decided opening leaves zero bytes"""
    K, vecs, key = kzg
    buf, mem = Z.batch(vecs, len(vecs), stride=199)
    r = pkg.dbg_kzg_fold(key, buf, n=len(vecs), stride=199, flags=pkg.FLAG_STRICT_SCALARS if strict else 0, device=-1)
    want = Z.expected_points(O, K, mem, strict)
    for i, v in enumerate(mem):
        assert r["status"][i] == Z.exact_status(K, v, strict), (v.name, r["status"][i])
        assert _points(r, i) == want[i], v.name
    if strict:
        assert V.NOT_MEMBER in {r["status"][i] for i, v in enumerate(mem) if v.name in ("z_ge_r", "y_ge_r", "both_ge_r", "strict_beats_curve")}
        assert all(r["status"][i] == V.NOT_MEMBER for i, v in enumerate(mem) if v.strict_err is not None)
    # the packed stride: same bytes
    buf2, _ = Z.batch(vecs, len(vecs))
    r2 = pkg.dbg_kzg_fold(key, buf2, flags=pkg.FLAG_STRICT_SCALARS if strict else 0, device=-1)
    assert all(r2[k] == r[k] for k in ("f", "h", "inf", "status"))


def _weights(rng, n):
    return ([1, 3, 2 ** 127 + 1, 2 ** 128 - 1] + [rng.randrange(2 ** 128) | 1 for _ in range(n)])[:n]


def test_host_compile_weighted_points(pkg, O, kzg):
    """explicit weights 1, 3, 2^127 + 1, 2^128 - 1 and random odd ones: F'_i = r_i F_i and H'_i = -r_i H_i from the oracle, and the status bytes the weighted path
    gives under these weights"""
    K, vecs, key = kzg
    # rotated so that the four special weights meet openings that reach the pairing with H != identity
    buf, mem = Z.batch(vecs, len(vecs))
    ws = _weights(random.Random(0x77), len(mem))
    assert all(Z.exact_status(K, v) in (V.ACCEPT, V.REJECT) and v.h for v in mem[:3])
    r = pkg.dbg_kzg_fold(key, buf, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    want = Z.expected_points(O, K, mem, weights=ws)
    for i, v in enumerate(mem):
        assert _points(r, i) == want[i], (v.name, ws[i])
    st, groups, failed = Z.expected_rlc(O, K, mem, ws)
    assert r["status"] == st == bytes(Z.exact_status(K, v) for v in mem) and failed == 1
    assert [(a, b, tuple(c), d) for a, b, c, d in r["groups"]] == groups
    # an even weight is forced odd: the same bytes as its odd neighbour
    r_even = pkg.dbg_kzg_fold(key, buf, weights=[w & ~1 if i % 2 else w for i, w in enumerate(ws)], flags=pkg.FLAG_RLC, device=-1)
    assert r_even["f"] == r["f"] and r_even["h"] == r["h"]


@pytest.mark.parametrize("n", (64, 65, 130))
def test_host_compile_group_sums(pkg, O, kzg, n):
    """groups of 64 with decided openings and identities inside, a partial last group: the sums of the weighted points of the pending openings and each group's verdict;
    a group of valid openings alone passes, and null weights are all 1"""
    K, vecs, key = kzg
    valid = [v for v in vecs if Z.exact_status(K, v) == V.ACCEPT]
    # group 0: every class; group 1 (n > 64): openings that verify, identities and loader errors among them -- it passes; group 2: a lone REJECT and a valid one
    mem = [vecs[i % len(vecs)] for i in range(64)]
    errs = [v for v in vecs if v.err is not None]
    mem += [(errs[i % len(errs)] if i % 9 == 4 else valid[i % len(valid)]) for i in range(64)]
    mem += [next(v for v in vecs if v.name == "value_plus_one"), valid[0]]
    mem = mem[:n]
    buf = b"".join(v.rec for v in mem)
    ws = _weights(random.Random(n), n)
    r = pkg.dbg_kzg_fold(key, buf, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    st, groups, failed = Z.expected_rlc(O, K, mem, ws)
    assert [(a, b, tuple(c), d) for a, b, c, d in r["groups"]] == groups
    assert r["status"] == st == bytes(Z.exact_status(K, v) for v in mem)
    assert [g[3] for g in groups] == [V.REJECT, V.ACCEPT, V.REJECT][:len(groups)] and failed == (2 if n > 128 else 1)
    assert any(g[0] != bytes(64) for g in groups)
    r1 = pkg.dbg_kzg_fold(key, buf, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    st1, groups1, _ = Z.expected_rlc(O, K, mem, [1] * n)
    assert [(a, b, tuple(c), d) for a, b, c, d in r1["groups"]] == groups1 and r1["status"] == st1


def test_host_compile_cancelling_forgeries_pass_under_unit_weights(pkg, O, kzg):
    """the vectors of the GPU forgery test are right: with all weights 1 the two errors cancel and the group passes -- and with distinct weights it does not"""
    K, vecs, key = kzg
    rng = random.Random(0xF0)
    va, vb = Z.forgery_pair(O, K, rng)
    valid = [v for v in vecs if Z.exact_status(K, v) == V.ACCEPT]
    mem = [valid[i % len(valid)] for i in range(20)]
    mem[3], mem[11] = va, vb
    buf = b"".join(v.rec for v in mem)
    r = pkg.dbg_kzg_fold(key, buf, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    assert r["groups"][0][3] == V.ACCEPT and r["status"] == bytes([V.ACCEPT] * 20)
    ws = _weights(random.Random(1), 20)
    r = pkg.dbg_kzg_fold(key, buf, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    assert r["groups"][0][3] == V.REJECT and r["status"][3] == r["status"][11] == V.REJECT and r["status"].count(V.ACCEPT) == 18
    assert pkg.dbg_kzg_fold(key, buf, device=-1)["status"] == r["status"]


def test_identity_key_points(pkg, O):
    """a pair with an identity on either side contributes 1: g1 the identity drops the y term, g2 the identity leaves e(-H, tau_g2) alone"""
    K, vecs = Z.vectors(O)
    v = next(x for x in vecs if x.name == "valid0")
    _, key_g1 = pkg.kzg_key_prepare(bytes(64), K["g2"], K["tau_g2"])
    r = pkg.dbg_kzg_fold(key_g1, v.rec, device=-1)
    assert r["f"] == Z.g1_of(O, v.c + v.z * v.h) and r["status"] == bytes([V.REJECT])
    _, key_g2 = pkg.kzg_key_prepare(K["g1"], bytes(128), K["tau_g2"])
    buf = v.rec + next(x for x in vecs if x.name == "h_identity_wrong").rec
    assert pkg.dbg_kzg_fold(key_g2, buf, device=-1)["status"] == bytes([V.REJECT, V.ACCEPT])      # H != O: not 1; H = O: both pairs contribute 1
    _, key_tau = pkg.kzg_key_prepare(K["g1"], K["g2"], bytes(128))
    assert pkg.dbg_kzg_fold(key_tau, v.rec + next(x for x in vecs if x.name == "f_identity").rec, device=-1)["status"] == bytes([V.REJECT, V.ACCEPT])


def test_argument_errors_touch_nothing(pkg, O, kzg):
    K, vecs, key = kzg
    L = pkg.lib()
    L.bn254_last_error.restype = C.c_char_p
    L.bn254_kzg_verify_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    L.bn254_kzg_verify_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    L.bn254_dbg_kzg_fold.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    st = (C.c_uint8 * 4)(*([0xEE] * 4))
    stp = C.cast(st, C.c_void_p)
    scratch = (C.c_uint8 * 1024)()
    sp = C.cast(scratch, C.c_void_p)
    item = vecs[0].rec * 2
    kbuf = C.create_string_buffer(key, len(key))          # stands for device memory in the device entry: never dereferenced before the device check
    kp, ip = C.cast(kbuf, C.c_void_p), C.cast(C.create_string_buffer(item, len(item)), C.c_void_p)

    def untouched():
        return bytes(st) == b"\xee" * 4

    def corrupt(off, value):
        b = bytearray(key)
        struct.pack_into("<I", b, off, value)
        return bytes(b)

    host = lambda k, o, s, n, status, flags: L.bn254_kzg_verify_batch(k, o, s, n, status, NO_SUCH_DEVICE, flags)
    probe = lambda k, o, s, n, status, flags: L.bn254_dbg_kzg_fold(k, o, s, n, None, flags, sp, sp, sp, status, None, NO_SUCH_DEVICE, 0)
    probe_host = lambda k, o, s, n, status, flags: L.bn254_dbg_kzg_fold(k, o, s, n, None, flags, sp, sp, sp, status, None, -1, 0)
    for name, call in (("host", host), ("probe", probe), ("probe_host", probe_host)):
        assert call(None, item, 192, 1, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(key, None, 192, 1, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(key, item, 192, 1, None, 0) == E_BAD_ARG and untouched(), name
        assert call(key, item, 191, 1, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(key, item, 192, 1, stp, 4) == E_BAD_ARG and call(key, item, 192, 1, stp, 8 | pkg.FLAG_RLC) == E_BAD_ARG and untouched(), name
        assert call(corrupt(0, MAGIC ^ 1), item, 192, 1, stp, 0) == E_BAD_ARG and untouched(), name
        assert b"magic" in L.bn254_last_error(), name
        assert call(corrupt(4, VERSION + 1), item, 192, 1, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(corrupt(HDR + G1_DIGITS + pkg.G2_PREPARED_LEN, 7), item, 192, 1, stp, 0) == E_BAD_ARG and untouched(), name      # the second record's magic word
        assert call(key, item, 2 ** 63, 3, stp, 0) == E_BAD_ARG and untouched(), name
        assert call(key, item, 192, 0, stp, 0) == 0 and call(None, None, 192, 0, None, pkg.FLAG_RLC) == 0 and untouched(), name      # n == 0
        if name != "probe_host":
            rc = call(key, item, 192, 2, stp, pkg.FLAG_RLC | pkg.FLAG_STRICT_SCALARS)                                                # past the argument checks: the device ordinal
            assert rc in (-1, -2) and untouched() and b"device" in L.bn254_last_error().lower(), name
    dev = lambda k, o, s, n, status, flags: L.bn254_kzg_verify_batch_device(k, o, s, n, status, NO_SUCH_DEVICE, None, flags)
    assert dev(None, ip, 192, 1, stp, 0) == E_BAD_ARG and dev(kp, None, 192, 1, stp, 0) == E_BAD_ARG and dev(kp, ip, 192, 1, None, 0) == E_BAD_ARG and untouched()
    assert dev(kp, ip, 100, 1, stp, 0) == E_BAD_ARG and dev(kp, ip, 192, 1, stp, 16) == E_BAD_ARG and untouched()
    assert dev(C.c_void_p(kp.value + 2), ip, 192, 1, stp, 0) == E_BAD_ARG and b"aligned" in L.bn254_last_error() and untouched()
    assert dev(kp, ip, 192, 0, stp, 0) == 0 and dev(None, None, 192, 0, None, 0) == 0 and untouched()
    rc = dev(kp, ip, 192, 2, stp, 0)
    assert rc in (-1, -2) and untouched() and b"device" in L.bn254_last_error().lower()
    # the probe's own rules: weights and group output need the flag, a forced form needs a device, one form number too many
    w = bytes(32)
    assert L.bn254_dbg_kzg_fold(key, item, 192, 2, w, 0, sp, sp, sp, stp, None, -1, 0) == E_BAD_ARG and untouched()
    assert L.bn254_dbg_kzg_fold(key, item, 192, 2, None, 0, sp, sp, sp, stp, sp, -1, 0) == E_BAD_ARG and untouched()
    assert L.bn254_dbg_kzg_fold(key, item, 192, 2, None, 0, sp, sp, sp, stp, None, -1, 1) == E_BAD_ARG and untouched()
    assert L.bn254_dbg_kzg_fold(key, item, 192, 2, None, 0, sp, sp, sp, stp, None, -1, 3) == E_BAD_ARG and untouched()
    assert L.bn254_dbg_kzg_fold(key, item, 192, 2, None, 0, None, sp, sp, stp, None, -1, 0) == E_BAD_ARG and untouched()


def test_knob_clamps_and_reads_back(pkg):
    before = pkg.kzg_params()
    try:
        assert before >= 64
        pkg.set_kzg_params(1000)
        assert pkg.kzg_params() == 1000
        pkg.set_kzg_params(-1)
        assert pkg.kzg_params() == 1000          # a negative value leaves it alone
        pkg.set_kzg_params(0)
        assert pkg.kzg_params() == 64            # never below 64
        pkg.set_kzg_params(63)
        assert pkg.kzg_params() == 64
        pkg.set_kzg_params(2 ** 40)
        assert pkg.kzg_params() == 2 ** 40
        assert len(pkg.kzg_state()) == 4
    finally:
        pkg.set_kzg_params(before)


def test_knob_initial_value_from_the_environment():
    """BN254_KZG_RLC_MIN gives the initial value (clamped), in a process of its own: the knob is read once, when the library is loaded"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = "import sys, importlib; sys.path.insert(0, %r); pkg = importlib.import_module('snark-bn254-verifier_amd'); print(pkg.kzg_params())" % root
    for env, want in (("12345", 12345), ("5", 64)):
        r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, env=dict(os.environ, BN254_KZG_RLC_MIN=env), timeout=300)
        assert r.returncode == 0 and int(r.stdout.split()[-1]) == want, r.stdout + r.stderr[-2000:]
