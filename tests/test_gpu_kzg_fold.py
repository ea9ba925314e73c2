"""Batch verification of KZG batch-opening proofs on the GPU (include/bn254_verify.h: bn254_kzg_verify_folded_batch, _device; the new kernel k_kzg_fold_load in front
of the kernels of the KZG batch): the vector classes of tests/kzg_fold_common.py at k = 1, 2, 3, 8 and the largest k, at batch sizes on both sides of the wavefront and
of the 256-thread block, packed and at a stride that is no multiple of 4 -- the digest gamma is reduced from, y^ = sum gamma^i y_i, the points the loader and the G1
walk leave and the status bytes against the host compile and the Python expectation, byte for byte.  The gamma and y^ comparison is the guard of the kernel's
digest-to-field step (the device self-test does not cover this kernel).  Then the public entries: strict scalars, both forms of the pairing launches, parity with
bn254_kzg_verify_batch at k = 1, the weighted path against the exact one with its counters, cancelling forgeries, a corrupted key, the enqueue-only entry."""
import random

import pytest

import kzg_common as Z
import kzg_fold_common as F
import pairing_batch_common as V
import test_gpu_pairing_batch as _PB

pytestmark = pytest.mark.gpu
LANES, COOP = 1, 2
MALFORMED = 6
SIZES = (1, 63, 64, 65, 257)
DL = F.MAIN_DATA_LEN
_SIDE = _PB._SIDE      # THE stream beside the default one, shared with the pairing tests (tests/test_gpu_pairing_batch.py)
_KEY = {}
_HOST = {}


def _key(pkg, O, k):
    if k not in _KEY:
        K, main, extras = F.vectors(O, k)
        st, key = pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"])
        assert st == V.ACCEPT
        _KEY[k] = (K, main, extras, key)
    return _KEY[k]


def _points(r, i):
    return r["f"][64 * i:64 * i + 64], r["h"][64 * i:64 * i + 64], tuple(r["inf"][2 * i:2 * i + 2])


def _host(pkg, O, k, n):
    """the host compile's answer for the batch of n records of the main family, once, itself held to the Python expectation"""
    if (k, n) not in _HOST:
        K, main, _, key = _key(pkg, O, k)
        buf, mem = F.batch(main, n)
        r = pkg.dbg_kzg_fold_proof(key, buf, k, DL, n=n, device=-1)
        want, fold = F.expected_points(O, K, mem), F.expected_fold(K, mem)
        for i, v in enumerate(mem):
            assert r["status"][i] == F.status(K, v) and _points(r, i) == want[i], v.name
            assert (r["gamma"][32 * i:32 * i + 32], r["yhat"][32 * i:32 * i + 32]) == fold[i], v.name
        _HOST[(k, n)] = (mem, r)
    return _HOST[(k, n)]


def _device_entry(pkg, key, buf, n, k, data_len=DL, stride=None, flags=0, fill=0xEE, reserve=None):
    import torch
    dev = torch.device("cuda:0")
    d_key = torch.frombuffer(bytearray(key), dtype=torch.uint8).to(dev)
    d_rec = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    d_status = torch.full((n,), fill, dtype=torch.uint8, device=dev)
    pkg.kzg_fold_reserve(n if reserve is None else reserve, k, device=0)
    torch.cuda.synchronize(dev)
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(device=dev))
    side = _SIDE[0]
    pkg.kzg_verify_folded_batch_device(d_key.data_ptr(), d_rec.data_ptr(), n, k, d_status.data_ptr(), data_len=data_len, stride=stride, device=0, stream=side.cuda_stream, flags=flags)
    side.synchronize()
    return bytes(d_status.cpu().numpy().tobytes())


@pytest.mark.parametrize("pad", (0, 5))
@pytest.mark.parametrize("k", F.KS)
@pytest.mark.parametrize("n", SIZES)
def test_values_and_status_against_host_compile_and_python(pkg, O, n, k, pad):
    """the probe on the device in both forms of the pairing that follows: the digest, y^, F, -H, the identity flags and the status bytes equal the host compile's, which
    equals the Python expectation; the public entry gives the same status bytes"""
    K, main, _, key = _key(pkg, O, k)
    mem, host = _host(pkg, O, k, n)
    stride = F.rec_len(k, DL) + pad
    buf, _ = F.batch(main, n, stride)
    if n >= 63:
        assert {F.status(K, v) for v in mem[:63]} == {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE} and len(main) <= 63      # every class inside the first wavefront
    for form in (LANES, COOP):
        dev = pkg.dbg_kzg_fold_proof(key, buf, k, DL, n=n, stride=stride, device=0, form=form)
        for name in ("gamma", "yhat", "status", "inf", "f", "h"):
            assert dev[name] == host[name], (n, k, pad, form, name)
    assert pkg.kzg_verify_folded_batch(key, buf, k, DL, n=n, stride=stride, device=0) == host["status"]


@pytest.mark.parametrize("k", F.KS)
def test_data_lengths_at_the_padding_edges(pkg, O, k):
    """the data lengths that end the hashed message at 55, 56, 63 and 0 mod 64, and 0 and 64 bytes of data: gamma on the device is hashlib's, through the probe (records
    staged at a padded stride) and through the device entry on the caller's packed buffer (dword loads where the record length allows, byte loads elsewhere)"""
    K, _, extras, key = _key(pkg, O, k)
    assert {(37 + 96 * k + dl) % 64 for dl, _ in extras} >= {55, 56, 63, 0}
    for dl, fam in extras:
        buf, mem = F.batch(fam, 66)
        want, fold = bytes(F.status(K, v) for v in mem), F.expected_fold(K, mem)
        dev = pkg.dbg_kzg_fold_proof(key, buf, k, dl, n=66, device=0)
        assert dev["status"] == want and set(want) == {V.ACCEPT, V.REJECT}, (k, dl)
        assert dev["gamma"] == b"".join(f[0] for f in fold) and dev["yhat"] == b"".join(f[1] for f in fold), (k, dl)
        assert _device_entry(pkg, key, buf, 66, k, data_len=dl) == want, (k, dl)


@pytest.mark.parametrize("k", (1, 3, 13))
def test_strict_scalars(pkg, O, k):
    K, main, _, key = _key(pkg, O, k)
    buf, mem = F.batch(main, 65)
    want = bytes(F.status(K, v, True) for v in mem)
    assert want != bytes(F.status(K, v) for v in mem)
    assert pkg.dbg_kzg_fold_proof(key, buf, k, DL, device=0, flags=pkg.FLAG_STRICT_SCALARS)["status"] == want
    assert pkg.kzg_verify_folded_batch(key, buf, k, DL, device=0, flags=pkg.FLAG_STRICT_SCALARS) == want
    assert _device_entry(pkg, key, buf, 65, k, flags=pkg.FLAG_STRICT_SCALARS) == want


@pytest.mark.parametrize("coop_max", (0, 30720))
def test_both_pairing_forms_and_three_ways_in_agree(pkg, O, coop_max):
    """host entry, device entry on a side stream, probe -- with the cooperative form of the pairing launches off and on"""
    before = pkg.pairing_params()
    try:
        pkg.set_pairing_params(coop_max)
        for k, n, pad in ((3, 65, 0), (8, 257, 3)):
            K, main, _, key = _key(pkg, O, k)
            mem, host = _host(pkg, O, k, n)
            stride = F.rec_len(k, DL) + pad
            buf, _ = F.batch(main, n, stride)
            want = host["status"]
            s0 = pkg.pairing_state()
            assert pkg.kzg_verify_folded_batch(key, buf, k, DL, n=n, stride=stride, device=0) == want
            s1 = pkg.pairing_state()
            assert (s1[0] - s0[0], s1[1] - s0[1]) == ((1, 0) if coop_max else (0, 1))      # the plan's choice of form applies
            assert _device_entry(pkg, key, buf, n, k, stride=stride) == want
            assert pkg.dbg_kzg_fold_proof(key, buf, k, DL, n=n, stride=stride, device=0)["status"] == want
    finally:
        pkg.set_pairing_params(before)


def test_one_digest_is_an_opening(pkg, O):
    """k = 1, data_len = 0: a record is an opening -- the status bytes of bn254_kzg_verify_batch on the same buffer, for kzg_common's openings (every class) and for this
    file's records"""
    K, vecs = Z.vectors(O)
    st, key = pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"])
    for stride in (192, 197):
        buf, mem = Z.batch(vecs, 130, stride)
        want = bytes(Z.exact_status(K, v) for v in mem)
        assert pkg.kzg_verify_batch(key, buf, n=130, stride=stride, device=0) == want
        assert pkg.kzg_verify_folded_batch(key, buf, 1, 0, n=130, stride=stride, device=0) == want
        strict = pkg.kzg_verify_batch(key, buf, n=130, stride=stride, device=0, flags=pkg.FLAG_STRICT_SCALARS)
        assert pkg.kzg_verify_folded_batch(key, buf, 1, 0, n=130, stride=stride, device=0, flags=pkg.FLAG_STRICT_SCALARS) == strict != want
    _, _, extras, _ = _key(pkg, O, 1)
    fam = dict(extras)[0]
    buf, mem = F.batch(fam, 70)
    assert pkg.kzg_verify_batch(key, buf, device=0) == pkg.kzg_verify_folded_batch(key, buf, 1, 0, device=0) == bytes(F.status(K, v) for v in mem)


def _rlc_batch(K, main, n, kind):
    valid = [v for v in main if F.status(K, v) == V.ACCEPT]
    if kind == "all_valid":
        mem = [valid[i % len(valid)] for i in range(n)]
    elif kind == "one_reject":       # one REJECT in the middle group, loader errors and identities in the groups that pass
        errs = [v for v in main if v.err is not None]
        mem = [(errs[i % len(errs)] if i % 11 == 5 else valid[i % len(valid)]) for i in range(n)]
        mid = ((n + 63) // 64 // 2) * 64 + 7
        mem[min(mid, n - 1)] = next(v for v in main if v.name == "value0_plus_one")
    else:                            # every class in every group
        mem = [main[i % len(main)] for i in range(n)]
    return b"".join(v.rec for v in mem), mem


@pytest.mark.parametrize("k", (1, 3, 13))
@pytest.mark.parametrize("n", (64, 65, 129, 320))
def test_rlc_equals_exact_and_counts(pkg, O, n, k):
    """set_kzg_params(64): an all-valid batch, one REJECT in the middle group (with loader errors and identities around it), every class everywhere, a partial last
    group -- the status bytes of the exact path, the joint check counted with exactly the expected launches, groups and failed groups; the knob above n: the exact path"""
    K, main, _, key = _key(pkg, O, k)
    before = pkg.kzg_params()
    try:
        for kind in ("all_valid", "one_reject", "classes"):
            buf, mem = _rlc_batch(K, main, n, kind)
            want = bytes(F.status(K, v) for v in mem)
            groups = (n + 63) // 64
            failing = {i // 64 for i, v in enumerate(mem) if want[i] == V.REJECT}
            assert (len(failing) >= groups - 1) if kind == "classes" else len(failing) == {"all_valid": 0, "one_reject": 1}[kind]
            pkg.set_kzg_params(64)
            s0 = pkg.kzg_state()
            got = pkg.kzg_verify_folded_batch(key, buf, k, DL, device=0, flags=pkg.FLAG_RLC)
            s1 = pkg.kzg_state()
            assert got == want, (n, k, kind)
            assert tuple(b - a for a, b in zip(s0, s1)) == (1, groups, len(failing), 0), (n, k, kind)
            if kind == "one_reject":
                assert _device_entry(pkg, key, buf, n, k, flags=pkg.FLAG_RLC) == want
                s2 = pkg.kzg_state()
                assert tuple(b - a for a, b in zip(s1, s2)) == (1, groups, 1, 0)
                assert pkg.kzg_verify_folded_batch(key, buf, k, DL, device=0) == want                      # the exact path's bytes
                pkg.set_kzg_params(n + 1)
                s3 = pkg.kzg_state()
                assert pkg.kzg_verify_folded_batch(key, buf, k, DL, device=0, flags=pkg.FLAG_RLC) == want
                assert tuple(b - a for a, b in zip(s3, pkg.kzg_state())) == (0, 0, 0, 1)     # the knob above n: the exact path
    finally:
        pkg.set_kzg_params(before)


@pytest.mark.parametrize("k", (2, 13))
def test_rlc_probe_values_on_the_device(pkg, O, k):
    """the weighted points, the group sums and the groups' verdicts under explicit weights: the kernels against the host compile and the Python expectation"""
    K, main, _, key = _key(pkg, O, k)
    n = 130
    buf, mem = F.batch(main, n)
    rng = random.Random(0x130 + k)
    ws = [1, 3, 2 ** 127 + 1, 2 ** 128 - 1] + [rng.randrange(2 ** 128) | 1 for _ in range(n - 4)]
    host = pkg.dbg_kzg_fold_proof(key, buf, k, DL, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    st, groups, failed = F.expected_rlc(O, K, mem, ws)
    assert host["status"] == st and [(a, b, tuple(c), d) for a, b, c, d in host["groups"]] == groups and failed >= 2
    want = F.expected_points(O, K, mem, weights=ws)
    assert all(_points(host, i) == want[i] for i in range(n))
    for form in (LANES, COOP):
        dev = pkg.dbg_kzg_fold_proof(key, buf, k, DL, weights=ws, flags=pkg.FLAG_RLC, device=0, form=form, want_groups=True)
        for name in ("gamma", "yhat", "status", "inf", "f", "h", "groups"):
            assert dev[name] == host[name], (form, name)


@pytest.mark.parametrize("k", (1, 3))
def test_cancelling_forgeries_are_rejected(pkg, O, k):
    """one group holds two records whose quotients are off by amounts that cancel.  With all weights 1 the errors cancel -- the probe shows the group passing, so the
    vectors are right -- and the product entry, whose weights are fresh per call and per record, answers REJECT for both in 10 consecutive calls"""
    K, main, _, key = _key(pkg, O, k)
    va, vb = F.forgery_pair(O, K, random.Random(0xF06 + k), k)
    valid = [v for v in main if F.status(K, v) == V.ACCEPT]
    mem = [valid[i % len(valid)] for i in range(64)]
    mem[9], mem[40] = va, vb
    buf = b"".join(v.rec for v in mem)
    unit = pkg.dbg_kzg_fold_proof(key, buf, k, DL, flags=pkg.FLAG_RLC, device=0, want_groups=True)
    assert unit["groups"][0][3] == V.ACCEPT and unit["status"] == bytes([V.ACCEPT] * 64)
    want = bytes(V.REJECT if i in (9, 40) else V.ACCEPT for i in range(64))
    before = pkg.kzg_params()
    try:
        pkg.set_kzg_params(64)
        s0 = pkg.kzg_state()
        for _ in range(10):
            assert pkg.kzg_verify_folded_batch(key, buf, k, DL, device=0, flags=pkg.FLAG_RLC) == want
        assert tuple(b - a for a, b in zip(s0, pkg.kzg_state())) == (10, 10, 10, 0)
    finally:
        pkg.set_kzg_params(before)


def test_corrupted_key_through_the_device_entry(pkg, O):
    """the device entry cannot read the key on the host: the loader kernel reads the header words, every record ends MALFORMED; the next call with the sound key
    answers right"""
    k = 3
    K, main, _, key = _key(pkg, O, k)
    mem, host = _host(pkg, O, k, 65)
    buf, _ = F.batch(main, 65)
    for off in (0, 4, 16 + 72, 16 + 72 + pkg.G2_PREPARED_LEN + 4):      # the key's magic word and version, the first record's magic word, the second's version
        bad = bytearray(key)
        bad[off] ^= 1
        assert _device_entry(pkg, bytes(bad), buf, 65, k) == bytes([MALFORMED] * 65), off
    before = pkg.kzg_params()
    try:
        pkg.set_kzg_params(64)
        bad = bytearray(key); bad[0] ^= 1
        assert _device_entry(pkg, bytes(bad), buf, 65, k, flags=pkg.FLAG_RLC) == bytes([MALFORMED] * 65)
    finally:
        pkg.set_kzg_params(before)
    assert _device_entry(pkg, key, buf, 65, k) == host["status"]


def test_enqueue_only_entry(pkg, O):
    """after kzg_fold_reserve(n, k) the exact device entry only enqueues on the caller's stream: the status bytes are written by that stream's work (whatever the fill
    value was) and the reservation serves a smaller batch as well"""
    k = 8
    K, main, _, key = _key(pkg, O, k)
    mem, host = _host(pkg, O, k, 257)
    buf, _ = F.batch(main, 257)
    for fill in (0xEE, 0x00):
        assert _device_entry(pkg, key, buf, 257, k, fill=fill, reserve=300) == host["status"]
    mem65, host65 = _host(pkg, O, k, 65)
    buf65, _ = F.batch(main, 65)
    assert _device_entry(pkg, key, buf65, 65, k, reserve=300) == host65["status"]
