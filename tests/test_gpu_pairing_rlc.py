"""BN254_FLAG_RLC on the pairing batch on the GPU (bn254_pairing_check_batch_flags, _device; bn254_dbg_pairing_batch_rlc): the kernels (k_pairing_rlc_weigh,
k_miller_run_sub, k_pairing_rlc_group_sums, k_pairing_rlc_group_prod and the group check in both forms) against the host compile of the same bodies byte for byte --
item GT, group GT, group status, status -- and the product entries against the exact entry and the vectors' statuses, with the counters of bn254_pairing_rlc_state.
The host compile itself is held to the oracle in tests/test_pairing_rlc_cpu.py."""
import pytest

import pairing_batch_common as V
import pairing_rlc_common as R
import pairing_shared_common as S

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)


def _device_entry(pkg, buf, k, mask, prep, n, flags, fill=0xEE, reserve=True):
    import torch
    dev = torch.device("cuda:0")
    d_items = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    d_prep = torch.frombuffer(bytearray(prep if prep else bytes(4)), dtype=torch.uint8).to(dev)
    assert d_prep.data_ptr() % 4 == 0
    d_status = torch.full((n,), fill, dtype=torch.uint8, device=dev)
    if reserve:
        pkg.pairing_reserve(n, device=0)
    # on the stream the process already has: a stream of this module's own would move the streams that later tests create to other hardware queues
    stream = torch.cuda.current_stream(dev)
    torch.cuda.synchronize(dev)
    pkg.pairing_check_batch_shared_device(d_items.data_ptr(), k, mask, d_prep.data_ptr() if mask else 0, n, d_status.data_ptr(), device=0, stream=stream.cuda_stream, flags=flags)
    stream.synchronize()
    return bytes(d_status.cpu().numpy().tobytes())


@pytest.fixture(autouse=True)
def _every_shape_honoured(pkg):
    """the product tests run the joint check at every shape: by default a shape with a variable position takes the exact path (test_default_shape_rule)"""
    was = pkg.dbg_set_pairing_rlc_max_var(8)
    yield
    pkg.dbg_set_pairing_rlc_max_var(was)


def test_default_shape_rule(pkg, O):
    """by default the flag is honoured for shapes without a variable position only: (2, 0b10) at 130 items above the knob counts as an exact launch, (2, 0b11) as a joint one"""
    was = pkg.pairing_rlc_params()
    pkg.dbg_set_pairing_rlc_max_var(-1)
    try:
        pkg.set_pairing_rlc_params(64)
        for (k, mask), want_d in (((2, 0b10), (0, 0, 0, 1)), ((2, 0b11), (1, 3, None, 0))):
            _, vecs = S.vectors(O, k, mask)
            items, want = R.build(vecs, R.layout(vecs, 130, "one_reject"), k, mask)
            s0 = pkg.pairing_rlc_state()
            assert pkg.pairing_check_batch_shared(items, k, mask, R.prepared_of(pkg, O, k, mask), n=130, device=0, flags=pkg.FLAG_RLC) == want
            d = tuple(b - a for a, b in zip(s0, pkg.pairing_rlc_state()))
            assert all(x is None or x == y for x, y in zip(want_d, d)), d
    finally:
        pkg.set_pairing_rlc_params(was)


def _failed_groups(want):
    """groups that hold a pending item that is not ACCEPT"""
    return sum(1 for g in range((len(want) + 63) // 64) if V.REJECT in want[64 * g:64 * g + 64])


@pytest.mark.parametrize("k,mask", R.SHAPES)
def test_kernels_against_the_host_compile(pkg, O, k, mask):
    _, vecs = S.vectors(O, k, mask)
    prep = R.prepared_of(pkg, O, k, mask)
    coop_max = pkg.pairing_params()
    try:
        for n in SIZES:
            for kind in R.LAYOUTS:
                idx = R.layout(vecs, n, kind)
                items, want = R.build(vecs, idx, k, mask)
                weights = R.weights_for(n, seed=n)
                host = pkg.dbg_pairing_batch_rlc(items, k, mask, prep, n=n, weights=weights, device=-1)
                assert host["status"] == want
                for knob in (0, coop_max):      # the lane form, then the plan's choice (the cooperative form at these sizes)
                    pkg.set_pairing_params(knob)
                    got = pkg.dbg_pairing_batch_rlc(items, k, mask, prep, n=n, weights=weights, device=0)
                    tag = (k, mask, n, kind, knob)
                    assert got["status"] == host["status"], tag
                    assert got["group_status"] == host["group_status"], tag
                    assert got["group_gt"] == host["group_gt"], tag
                    for i in range(n):      # an item that left before the groups were formed has no value
                        if want[i] in R.PENDING:
                            assert got["item_gt"][384 * i:384 * i + 384] == host["item_gt"][384 * i:384 * i + 384], tag + (i,)
    finally:
        pkg.set_pairing_params(coop_max)


@pytest.mark.parametrize("k,mask", R.SHAPES)
def test_product_entries(pkg, O, k, mask):
    """host and device entry with the flag honoured from 64 items on: the statuses of the exact entry on the same bytes and of the vectors; the counters"""
    _, vecs = S.vectors(O, k, mask)
    prep = R.prepared_of(pkg, O, k, mask)
    was = pkg.pairing_rlc_params()
    try:
        pkg.set_pairing_rlc_params(64)
        for n, kind in ((257, "mixed"), (130, "one_reject"), (65, "decided_group"), (63, "mixed")):
            idx = R.layout(vecs, n, kind)
            items, want = R.build(vecs, idx, k, mask)
            exact = pkg.pairing_check_batch_shared(items, k, mask, prep, n=n, device=0) if mask else pkg.pairing_check_batch(items, k, n=n, device=0)
            assert exact == want
            for entry in ("host", "device"):
                s0 = pkg.pairing_rlc_state()
                if entry == "host":
                    got = pkg.pairing_check_batch_shared(items, k, mask, prep, n=n, device=0, flags=pkg.FLAG_RLC)
                else:
                    got = _device_entry(pkg, items, k, mask, prep, n, pkg.FLAG_RLC)
                d = tuple(b - a for a, b in zip(s0, pkg.pairing_rlc_state()))
                assert got == want, (k, mask, n, kind, entry)
                if n >= 64:
                    assert d == (1, (n + 63) // 64, _failed_groups(want), 0), (k, mask, n, kind, entry, d)
                else:
                    assert d == (0, 0, 0, 1), (k, mask, n, kind, entry, d)      # below the knob: the exact launch
    finally:
        pkg.set_pairing_rlc_params(was)


@pytest.mark.parametrize("k,mask", ((2, 0b11), (2, 0b10)))
def test_group_stage_crosses_a_wavefront(pkg, O, k, mask):
    """4097 items, 65 groups: all valid except the last item, alone in the last group and rejected"""
    _, vecs = S.vectors(O, k, mask)
    prep = R.prepared_of(pkg, O, k, mask)
    ok = [i for i, v in enumerate(vecs) if v[0] == "identity"][0]
    bad = [i for i, v in enumerate(vecs) if v[0] == "identity_perturbed"][0]
    n = 4097
    items, want = R.build(vecs, [ok] * 4096 + [bad], k, mask)
    was = pkg.pairing_rlc_params()
    try:
        pkg.set_pairing_rlc_params(64)
        s0 = pkg.pairing_rlc_state()
        got = pkg.pairing_check_batch_shared(items, k, mask, prep, n=n, device=0, flags=pkg.FLAG_RLC)
        d = tuple(b - a for a, b in zip(s0, pkg.pairing_rlc_state()))
        assert got == want and want == bytes([V.ACCEPT] * 4096 + [V.REJECT])
        assert d == (1, 65, 1, 0)
    finally:
        pkg.set_pairing_rlc_params(was)


@pytest.mark.parametrize("shared_first", (True, False))
def test_cancelling_forgery_through_the_product(pkg, O, shared_first):
    """the cancelling pair inside a group of valid items, the real draw: both rejected in 20 consecutive calls (a pass would take r_a == r_b mod r)"""
    (k, mask), recs, honest, forged = R.forgery(pkg, O, shared_first)
    rec = len(honest) // 2
    mem = [honest[:rec] if i % 2 == 0 else honest[rec:] for i in range(64)]
    mem[9], mem[40] = forged[:rec], forged[rec:]
    buf = b"".join(mem)
    ones = (1).to_bytes(16, "big") * 64
    unit = pkg.dbg_pairing_batch_rlc(buf, k, mask, recs, n=64, weights=ones, device=0)
    assert unit["group_status"] == bytes([V.ACCEPT]) and unit["status"] == bytes([V.ACCEPT] * 64)      # with equal weights the forgery passes
    want = bytes(V.REJECT if i in (9, 40) else V.ACCEPT for i in range(64))
    was = pkg.pairing_rlc_params()
    try:
        pkg.set_pairing_rlc_params(64)
        s0 = pkg.pairing_rlc_state()
        for _ in range(20):
            assert pkg.pairing_check_batch_shared(buf, k, mask, recs, n=64, device=0, flags=pkg.FLAG_RLC) == want
        assert tuple(b - a for a, b in zip(s0, pkg.pairing_rlc_state())) == (20, 20, 20, 0)
    finally:
        pkg.set_pairing_rlc_params(was)


def test_corrupted_record_through_the_device_entry(pkg, O):
    """a prepared record of another magic word, on the device where the host cannot see it: every item MALFORMED, no group fails, no table is read"""
    k, mask = 4, 0b1110
    _, vecs = S.vectors(O, k, mask)
    prep = bytearray(R.prepared_of(pkg, O, k, mask))
    prep[pkg.G2_PREPARED_LEN] ^= 1      # the second record's magic word
    n = 130
    items, _ = R.build(vecs, R.layout(vecs, n, "mixed"), k, mask)
    was = pkg.pairing_rlc_params()
    try:
        pkg.set_pairing_rlc_params(64)
        s0 = pkg.pairing_rlc_state()
        got = _device_entry(pkg, items, k, mask, bytes(prep), n, pkg.FLAG_RLC)
        d = tuple(b - a for a, b in zip(s0, pkg.pairing_rlc_state()))
        assert got == bytes([pkg.ERR_MALFORMED] * n)
        # the joint launch ran; out[1] counts the groups of the launch (3 here), whether or not one holds a pending item: none did, so no group was checked by a
        # pairing and none failed
        assert d == (1, 3, 0, 0)
    finally:
        pkg.set_pairing_rlc_params(was)


def test_enqueue_only_below_the_knob(pkg, O):
    """with rlc_min above n the device entry with the flag is the exact entry: after pairing_reserve(n) it only enqueues on the caller's stream (the status bytes are
    written by that stream's work whatever the fill value was) and the state moves out[3] alone"""
    k, mask = 2, 0b10
    _, vecs = S.vectors(O, k, mask)
    prep = R.prepared_of(pkg, O, k, mask)
    n = 257
    items, want = R.build(vecs, R.layout(vecs, n, "mixed"), k, mask)
    was = pkg.pairing_rlc_params()
    try:
        pkg.set_pairing_rlc_params(n + 1)
        pkg.pairing_reserve(300, device=0)
        for fill in (0xEE, 0x00):
            s0 = pkg.pairing_rlc_state()
            assert _device_entry(pkg, items, k, mask, prep, n, pkg.FLAG_RLC, fill=fill, reserve=False) == want
            assert tuple(b - a for a, b in zip(s0, pkg.pairing_rlc_state())) == (0, 0, 0, 1)
        s0 = pkg.pairing_rlc_state()
        assert pkg.pairing_check_batch_shared(items, k, mask, prep, n=n, device=0, flags=pkg.FLAG_RLC) == want
        assert tuple(b - a for a, b in zip(s0, pkg.pairing_rlc_state())) == (0, 0, 0, 1)
        # flags == 0 through the new symbols: the existing entry, no counter of this one moves
        import ctypes as C
        import sys
        L = sys.modules[pkg.__name__ + ".binding"]._shared_lib()
        st = (C.c_uint8 * n)()
        s0 = pkg.pairing_rlc_state()
        assert L.bn254_pairing_check_batch_flags(items, len(items) // n, k, mask, prep, n, st, 0, 0) == 0 and bytes(st) == want
        assert pkg.pairing_rlc_state() == s0
    finally:
        pkg.set_pairing_rlc_params(was)
