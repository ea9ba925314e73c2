"""Batch verification of KZG openings on the GPU (include/bn254_verify.h: bn254_kzg_verify_batch, _device; kernels k_kzg_load, k_g1_msm_rows, k_g1_sum_affine,
k_kzg_ident, the pairing batch behind its load step; weighted: k_plonk_group_sums / k_plonk_group_scatter): the vector classes of tests/kzg_common.py, all of them
inside one wavefront, at batch sizes on both sides of the wavefront and of the 256-thread block -- the points the loader and the G1 walk leave and the status bytes
against the host compile and the oracle, byte for byte; the three ways in; the restated items through the existing shared-G2 entry; the weighted path against the
exact one, with its counters; forgeries whose errors cancel under constant weights; a corrupted key; the enqueue-only entry."""
import random

import pytest

import kzg_common as Z
import pairing_batch_common as V
import test_gpu_pairing_batch as _PB

pytestmark = pytest.mark.gpu
LANES, COOP = 1, 2
MALFORMED = 6
SIZES = (1, 63, 64, 65, 257)
_SIDE = _PB._SIDE      # THE stream beside the default one, shared with the pairing tests: every stream a process creates takes a share of the runtime's few hardware
                       # queues (tests/test_gpu_pairing_batch.py), and the Groth16 tests behind this file measure whether their sub-batch streams overlap
_KEY = {}
_HOST = {}


def _key(pkg, O):
    if not _KEY:
        K, vecs = Z.vectors(O)
        st, key = pkg.kzg_key_prepare(K["g1"], K["g2"], K["tau_g2"])
        assert st == V.ACCEPT
        _KEY["k"] = (K, vecs, key)
    return _KEY["k"]


def _host(pkg, O, n, stride):
    """the host compile's answer for the batch of n openings at `stride`, once"""
    if (n, stride) not in _HOST:
        K, vecs, key = _key(pkg, O)
        buf, mem = Z.batch(vecs, n, stride)
        r = pkg.dbg_kzg_fold(key, buf, n=n, stride=stride, device=-1)
        want = Z.expected_points(O, K, mem)
        for i, v in enumerate(mem):      # the reference itself against the oracle
            assert r["status"][i] == Z.exact_status(K, v) and (r["f"][64 * i:64 * i + 64], r["h"][64 * i:64 * i + 64], tuple(r["inf"][2 * i:2 * i + 2])) == want[i], v.name
        _HOST[(n, stride)] = (buf, mem, r)
    return _HOST[(n, stride)]


def _device_entry(pkg, key, buf, n, stride=192, flags=0, fill=0xEE):
    import torch
    dev = torch.device("cuda:0")
    d_key = torch.frombuffer(bytearray(key), dtype=torch.uint8).to(dev)
    d_open = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    d_status = torch.full((n,), fill, dtype=torch.uint8, device=dev)
    pkg.kzg_reserve(n, device=0)
    torch.cuda.synchronize(dev)
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(device=dev))
    side = _SIDE[0]
    pkg.kzg_verify_batch_device(d_key.data_ptr(), d_open.data_ptr(), n, d_status.data_ptr(), stride=stride, device=0, stream=side.cuda_stream, flags=flags)
    side.synchronize()
    return bytes(d_status.cpu().numpy().tobytes())


@pytest.mark.parametrize("stride", (192, 197))
@pytest.mark.parametrize("n", SIZES)
def test_values_and_status_against_host_compile_and_oracle(pkg, O, n, stride):
    """the probe on the device in both forms of the pairing that follows: F_i, -H_i, their identity flags and the status bytes equal the host compile's, which equals
    the oracle's (stride 197: the loader's byte loads)"""
    K, vecs, key = _key(pkg, O)
    buf, mem, host = _host(pkg, O, n, stride)
    if n >= 63:
        assert Z.status_classes(K, mem[:63]) == {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE} and len(vecs) <= 63      # every class inside the first wavefront
    for form in (LANES, COOP):
        dev = pkg.dbg_kzg_fold(key, buf, n=n, stride=stride, device=0, form=form)
        for k in ("status", "inf", "f", "h"):
            assert dev[k] == host[k], (n, stride, form, k)


def test_strict_scalars(pkg, O):
    K, vecs, key = _key(pkg, O)
    buf, mem = Z.batch(vecs, 65)
    want = bytes(Z.exact_status(K, v, True) for v in mem)
    assert want != bytes(Z.exact_status(K, v) for v in mem)
    assert pkg.dbg_kzg_fold(key, buf, device=0, flags=pkg.FLAG_STRICT_SCALARS)["status"] == want
    assert pkg.kzg_verify_batch(key, buf, device=0, flags=pkg.FLAG_STRICT_SCALARS) == want


@pytest.mark.parametrize("coop_max", (0, 30720))
def test_three_ways_in_agree(pkg, O, coop_max):
    """host entry, device entry on a side stream, probe -- with the cooperative form of the pairing launches off and on"""
    K, vecs, key = _key(pkg, O)
    before = pkg.pairing_params()
    try:
        pkg.set_pairing_params(coop_max)
        for n, stride in ((65, 192), (257, 200)):
            buf, mem, host = _host(pkg, O, n, 192)
            if stride != 192:
                buf, _ = Z.batch(vecs, n, stride)
            want = host["status"]
            s0 = pkg.pairing_state()
            assert pkg.kzg_verify_batch(key, buf, n=n, stride=stride, device=0) == want
            s1 = pkg.pairing_state()
            assert (s1[0] - s0[0], s1[1] - s0[1]) == ((1, 0) if coop_max else (0, 1))      # the plan's choice of form applies
            assert _device_entry(pkg, key, buf, n, stride) == want
            assert pkg.dbg_kzg_fold(key, buf, n=n, stride=stride, device=0)["status"] == want
    finally:
        pkg.set_pairing_params(before)


def test_against_the_existing_shared_entry(pkg, O):
    """the pending openings restated on the host as items (F_i, -H_i) give the same bytes through bn254_pairing_check_batch_shared with the key's two points"""
    K, vecs, key = _key(pkg, O)
    buf, mem, host = _host(pkg, O, 65, 192)
    pts = Z.expected_points(O, K, mem)
    pend = [i for i, v in enumerate(mem) if Z.exact_status(K, v) in (V.ACCEPT, V.REJECT)]
    items = b"".join(pts[i][0] + pts[i][1] for i in pend)
    recs = [pkg.g2_prepare(K["g2"])[1], pkg.g2_prepare(K["tau_g2"])[1]]
    got = pkg.pairing_check_batch_shared(items, 2, 0b11, recs, device=0)
    assert got == bytes(host["status"][i] for i in pend)
    assert pkg.kzg_verify_batch(key, buf, device=0) == host["status"]


def _rlc_batch(O, K, vecs, n, kind):
    valid = [v for v in vecs if Z.exact_status(K, v) == V.ACCEPT]
    if kind == "all_valid":
        mem = [valid[i % len(valid)] for i in range(n)]
    elif kind == "one_reject":       # one REJECT in the middle group, loader errors and identities in the groups that pass
        errs = [v for v in vecs if v.err is not None]
        mem = [(errs[i % len(errs)] if i % 11 == 5 else valid[i % len(valid)]) for i in range(n)]
        mid = ((n + 63) // 64 // 2) * 64 + 7
        mem[min(mid, n - 1)] = next(v for v in vecs if v.name == "value_plus_one")
    else:                            # every class in every group
        mem = [vecs[i % len(vecs)] for i in range(n)]
    return b"".join(v.rec for v in mem), mem


@pytest.mark.parametrize("n", (64, 65, 129, 257, 320))
def test_rlc_equals_exact_and_counts(pkg, O, n):
    """set_kzg_params(64): an all-valid batch, one REJECT in the middle group (with loader errors and identities around it), every class everywhere, a partial last
    group -- the status bytes of the exact entry, the joint check counted with exactly the expected number of failed groups; the knob above n: the exact path"""
    K, vecs, key = _key(pkg, O)
    before = pkg.kzg_params()
    try:
        for kind in ("all_valid", "one_reject", "classes"):
            buf, mem = _rlc_batch(O, K, vecs, n, kind)
            want = bytes(Z.exact_status(K, v) for v in mem)
            groups = (n + 63) // 64
            failing = {i // 64 for i, v in enumerate(mem) if want[i] == V.REJECT}
            assert (len(failing) >= groups - 1) if kind == "classes" else len(failing) == {"all_valid": 0, "one_reject": 1}[kind]      # (a last group of one decided opening passes)
            pkg.set_kzg_params(64)
            s0 = pkg.kzg_state()
            got = pkg.kzg_verify_batch(key, buf, device=0, flags=pkg.FLAG_RLC)
            s1 = pkg.kzg_state()
            assert got == want, (n, kind)
            assert tuple(b - a for a, b in zip(s0, s1)) == (1, groups, len(failing), 0), (n, kind)
            if kind == "one_reject":
                assert _device_entry(pkg, key, buf, n, flags=pkg.FLAG_RLC) == want
                s2 = pkg.kzg_state()
                assert tuple(b - a for a, b in zip(s1, s2)) == (1, groups, 1, 0)
                assert pkg.kzg_verify_batch(key, buf, device=0) == want                      # the exact entry's bytes
                pkg.set_kzg_params(n + 1)
                s3 = pkg.kzg_state()
                assert pkg.kzg_verify_batch(key, buf, device=0, flags=pkg.FLAG_RLC) == want
                assert tuple(b - a for a, b in zip(s3, pkg.kzg_state())) == (0, 0, 0, 1)     # the knob above n: the exact path
    finally:
        pkg.set_kzg_params(before)


def test_rlc_probe_values_on_the_device(pkg, O):
    """the weighted points, the group sums and the groups' verdicts under explicit weights: the kernels against the host compile and the oracle"""
    K, vecs, key = _key(pkg, O)
    n = 130
    buf, mem = Z.batch(vecs, n)
    rng = random.Random(0x130)
    ws = [1, 3, 2 ** 127 + 1, 2 ** 128 - 1] + [rng.randrange(2 ** 128) | 1 for _ in range(n - 4)]
    host = pkg.dbg_kzg_fold(key, buf, weights=ws, flags=pkg.FLAG_RLC, device=-1, want_groups=True)
    st, groups, failed = Z.expected_rlc(O, K, mem, ws)
    assert host["status"] == st and [(a, b, tuple(c), d) for a, b, c, d in host["groups"]] == groups and failed == 3
    for form in (LANES, COOP):
        dev = pkg.dbg_kzg_fold(key, buf, weights=ws, flags=pkg.FLAG_RLC, device=0, form=form, want_groups=True)
        for k in ("status", "inf", "f", "h", "groups"):
            assert dev[k] == host[k], (form, k)


def test_cancelling_forgeries_are_rejected(pkg, O):
    """one group holds two openings that claim v_a + d and v_b - d.  With all weights 1 the errors cancel -- the probe shows the group passing, so the vectors are
    right -- and the product entry, whose weights are fresh per call and per opening, answers REJECT for both in 20 consecutive calls"""
    K, vecs, key = _key(pkg, O)
    rng = random.Random(0xF06)
    va, vb = Z.forgery_pair(O, K, rng)
    valid = [v for v in vecs if Z.exact_status(K, v) == V.ACCEPT]
    mem = [valid[i % len(valid)] for i in range(64)]
    mem[9], mem[40] = va, vb
    buf = b"".join(v.rec for v in mem)
    unit = pkg.dbg_kzg_fold(key, buf, flags=pkg.FLAG_RLC, device=0, want_groups=True)
    assert unit["groups"][0][3] == V.ACCEPT and unit["status"] == bytes([V.ACCEPT] * 64)
    want = bytes(V.REJECT if i in (9, 40) else V.ACCEPT for i in range(64))
    before = pkg.kzg_params()
    try:
        pkg.set_kzg_params(64)
        s0 = pkg.kzg_state()
        for _ in range(20):
            assert pkg.kzg_verify_batch(key, buf, device=0, flags=pkg.FLAG_RLC) == want
        s1 = pkg.kzg_state()
        assert tuple(b - a for a, b in zip(s0, s1)) == (20, 20, 20, 0)
    finally:
        pkg.set_kzg_params(before)


def test_corrupted_key_through_the_device_entry(pkg, O):
    """the device entry cannot read the key on the host: the loader kernel reads the header words, every opening ends MALFORMED; the next call with the sound key
    answers right"""
    K, vecs, key = _key(pkg, O)
    buf, mem, host = _host(pkg, O, 65, 192)
    for off in (0, 4, 16 + 72, 16 + 72 + pkg.G2_PREPARED_LEN + 4):      # the key's magic word and version, the first record's magic word, the second's version
        bad = bytearray(key)
        bad[off] ^= 1
        assert _device_entry(pkg, bytes(bad), buf, 65) == bytes([MALFORMED] * 65), off
    before = pkg.kzg_params()
    try:
        pkg.set_kzg_params(64)
        bad = bytearray(key); bad[0] ^= 1
        assert _device_entry(pkg, bytes(bad), buf, 65, flags=pkg.FLAG_RLC) == bytes([MALFORMED] * 65)
    finally:
        pkg.set_kzg_params(before)
    assert _device_entry(pkg, key, buf, 65) == host["status"]


def test_enqueue_only_entry(pkg, O):
    """after kzg_reserve(n) the exact device entry only enqueues on the caller's stream: the status bytes are written by that stream's work (whatever the fill value
    was) and the workspace of the reservation serves a smaller batch as well"""
    K, vecs, key = _key(pkg, O)
    buf, mem, host = _host(pkg, O, 257, 192)
    pkg.kzg_reserve(300, device=0)
    for fill in (0xEE, 0x00):
        assert _device_entry(pkg, key, buf, 257, fill=fill) == host["status"]
    buf65, _, host65 = _host(pkg, O, 65, 192)
    assert _device_entry(pkg, key, buf65, 65) == host65["status"]
