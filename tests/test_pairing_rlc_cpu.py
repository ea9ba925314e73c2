"""BN254_FLAG_RLC on the pairing batch (include/bn254_verify.h: bn254_pairing_check_batch_flags, _device, bn254_set_pairing_rlc_params) without a GPU: through
bn254_dbg_pairing_batch_rlc(device = -1) -- the HOST compile of the weight step (pb_rlc_weigh_item), the Miller run over the variable positions alone
(vm_miller_run_sub: vm_miller_run_var with a mask of the positions that take part), the group sums, the group product and the group check -- every group's GT value against the oracle's
product over the group's pending items of e(r_i P_ij, Q_ij) byte for byte, the group's verdict, the final status bytes against the exact definition, the order of the
r-torsion tests and the group values, the cancelling forgery, the argument errors of the two entries and the knob's clamps.
The counters of bn254_pairing_rlc_state move only when a launch runs, which takes a device: tests/test_gpu_pairing_rlc.py holds them."""
import ctypes as C

import pytest

import pairing_batch_common as V
import pairing_rlc_common as R
import pairing_shared_common as S

E_BAD_ARG = -1
NO_SUCH_DEVICE = 4097
SIZES = (1, 63, 64, 65, 130)


def _raw(pkg):
    import sys
    b = sys.modules[pkg.__name__ + ".binding"]
    b._pairing_lib()
    return b._shared_lib()


@pytest.mark.parametrize("k,mask", R.SHAPES)
def test_groups_against_the_oracle(pkg, O, k, mask):
    """group GT value == prod over pending items of prod_j e(r_i P_ij, Q_ij); group status ACCEPT exactly when it is 1; final status bytes the exact definition's"""
    _, vecs = S.vectors(O, k, mask)
    prepared = R.prepared_of(pkg, O, k, mask)
    seen = set()
    for n in SIZES:
        for kind in R.LAYOUTS:
            idx = R.layout(vecs, n, kind)
            items, want = R.build(vecs, idx, k, mask)
            weights = R.weights_for(n, seed=n)
            got = pkg.dbg_pairing_batch_rlc(items, k, mask, prepared, n=n, weights=weights)
            exp = R.expected_groups(O, vecs, idx, k, weights)
            for g, (gt, st) in enumerate(exp):
                assert got["group_gt"][384 * g:384 * g + 384] == gt, (k, mask, n, kind, g)
                assert got["group_status"][g] == st == (V.ACCEPT if gt == V.GT_ONE else V.REJECT), (k, mask, n, kind, g)
            assert got["status"] == want, (k, mask, n, kind)
            seen |= set(want)
            if kind == "one_reject" and n > 1:
                mid = ((n + 63) // 64) // 2
                assert [g for g, (_, st) in enumerate(exp) if st != V.ACCEPT] == [mid] and want.count(bytes([V.REJECT])) == 1
            if kind == "decided_group":
                assert exp[0] == (V.GT_ONE, V.ACCEPT) and not set(want[:64]) & set(R.PENDING)      # a group decided in phase 1: the empty product
            if kind == "mixed" and n >= 64:
                names = {vecs[j][0] for j in idx[:64]}
                assert all(any(nm.startswith(c) for nm in names) for c in S.classes_of(k, mask) if any(v[0].startswith(c) for v in vecs))
    assert seen == S.statuses_of(k, mask)


@pytest.mark.parametrize("k,mask", ((2, 0b10), (4, 0b1110)))
def test_item_values_are_the_weighted_items(pkg, O, k, mask):
    """out_item_gt: the final-exponentiated value of the item on its WEIGHTED points, for every item that reached the groups"""
    _, vecs = S.vectors(O, k, mask)
    n = 65
    idx = R.layout(vecs, n, "mixed")
    items, want = R.build(vecs, idx, k, mask)
    weights = R.weights_for(n, seed=7)
    got = pkg.dbg_pairing_batch_rlc(items, k, mask, R.prepared_of(pkg, O, k, mask), n=n, weights=weights)
    for i in range(n):
        if want[i] in R.PENDING:
            assert got["item_gt"][384 * i:384 * i + 384] == R.gt_of(O, *R.item_pairs(O, vecs[idx[i]], k, R.weight_at(weights, i))), i
        else:
            assert got["item_gt"][384 * i:384 * i + 384] == bytes(384), i


@pytest.mark.parametrize("k,mask", [s for s in R.SHAPES if S.variable_positions(*s)])
def test_subgroup_failure_leaves_its_group(pkg, O, k, mask):
    """an item with a G2 point off the r-torsion inside an otherwise valid group: the group is ACCEPT (the item is in neither the sums nor the product) and the item
    itself NOT_IN_SUBGROUP -- the group values are formed behind the r-torsion tests"""
    _, vecs = S.vectors(O, k, mask)
    ok = [i for i, v in enumerate(vecs) if v[0] == "identity"][0]
    off = [i for i, v in enumerate(vecs) if v[0] == "g2_outside_subgroup_variable"][0]
    n = 9
    idx = [off if i == 4 else ok for i in range(n)]
    items, want = R.build(vecs, idx, k, mask)
    got = pkg.dbg_pairing_batch_rlc(items, k, mask, R.prepared_of(pkg, O, k, mask), n=n, weights=R.weights_for(n))
    assert got["group_status"] == bytes([V.ACCEPT]) and got["group_gt"] == V.GT_ONE
    assert got["status"] == want and want[4] == V.NOT_IN_SUBGROUP and want.count(bytes([V.ACCEPT])) == n - 1


@pytest.mark.parametrize("shared_first", (True, False))
def test_cancelling_forgery(pkg, O, shared_first):
    """P_a0 + T and P_b0 - T against the same G2 point: the unweighted sum hides T (asserted: with all weights 1 the group passes), two different weights expose it"""
    (k, mask), recs, honest, forged = R.forgery(pkg, O, shared_first)
    ones = (1).to_bytes(16, "big") * 2
    acc = bytes([V.ACCEPT] * 2)
    got = pkg.dbg_pairing_batch_rlc(honest, k, mask, recs, n=2, weights=R.weights_for(2))
    assert got["status"] == acc and got["group_status"] == acc[:1]
    got = pkg.dbg_pairing_batch_rlc(forged, k, mask, recs, n=2, weights=ones)
    assert got["group_status"] == acc[:1] and got["group_gt"] == V.GT_ONE      # what makes the next assertion mean something
    got = pkg.dbg_pairing_batch_rlc(forged, k, mask, recs, n=2, weights=(3).to_bytes(16, "big") + (5).to_bytes(16, "big"))
    assert got["group_status"] == bytes([V.REJECT]) and got["status"] == bytes([V.REJECT] * 2)
    # each forged item alone is invalid under the exact definition
    assert pkg.dbg_pairing_batch_shared(forged, k, mask, recs, n=2, want_gt=False)[1] == bytes([V.REJECT] * 2)


def test_argument_errors(pkg, O):
    L = _raw(pkg)
    k, mask = 2, 0b10
    _, vecs = S.vectors(O, k, mask)
    prepared = R.prepared_of(pkg, O, k, mask)
    item = vecs[0][1]
    st = (C.c_uint8 * 4)(*([0xEE] * 4))
    untouched = lambda: bytes(st) == b"\xee" * 4
    RLC = pkg.FLAG_RLC
    host = lambda items, stride, np_, m, prep, n, status, flags: L.bn254_pairing_check_batch_flags(items, stride, np_, m, prep, n, status, NO_SUCH_DEVICE, flags)
    dev = lambda items, stride, np_, m, prep, n, status, flags: L.bn254_pairing_check_batch_flags_device(items, stride, np_, m, prep, n, status, NO_SUCH_DEVICE, None, flags)
    rec = len(item)
    for call in (host, dev):
        # unknown flag bits, with and without the known one
        for flags in (2, 4, RLC | 2, 0x80000000):
            if flags & ~RLC:
                assert call(item, rec, k, mask, prepared, 1, st, flags) == E_BAD_ARG and untouched(), flags
        # those of the shared entry, with the flag set
        assert call(item, rec, 0, 0, None, 1, st, RLC) == E_BAD_ARG
        assert call(item, rec, 9, 0, None, 1, st, RLC) == E_BAD_ARG
        assert call(item, rec, k, 0b100, prepared, 1, st, RLC) == E_BAD_ARG
        assert call(item, rec, k, mask, None, 1, st, RLC) == E_BAD_ARG
        assert call(item, rec - 1, k, mask, prepared, 1, st, RLC) == E_BAD_ARG
        assert call(item, 192 * k - 1, k, 0, None, 1, st, RLC) == E_BAD_ARG
        assert call(None, rec, k, mask, prepared, 1, st, RLC) == E_BAD_ARG
        assert call(item, rec, k, mask, prepared, 1, None, RLC) == E_BAD_ARG
        assert call(item, 2 ** 63, k, mask, prepared, 4, st, RLC) == E_BAD_ARG
        assert untouched()
        # nothing to do: no device is touched
        assert call(item, rec, k, mask, prepared, 0, st, RLC) == 0 and untouched()
    bad = bytearray(prepared); bad[0] ^= 1
    assert host(item, rec, k, mask, bytes(bad), 1, st, RLC) == E_BAD_ARG and untouched()
    # the probe's own rules
    sp = C.cast(st, C.c_void_p)
    assert L.bn254_dbg_pairing_batch_rlc(item, rec, k, mask, prepared, 1, None, None, None, None, sp, -2, 0) == E_BAD_ARG
    assert L.bn254_dbg_pairing_batch_rlc(item, rec, k, mask, prepared, 1, None, None, None, None, sp, -1, 1) == E_BAD_ARG
    assert L.bn254_dbg_pairing_batch_rlc(item, rec, k, mask, prepared, 1, None, None, None, None, sp, -1, 3) == E_BAD_ARG and untouched()


def test_knob_clamps(pkg):
    was = pkg.pairing_rlc_params()
    try:
        assert was >= 64
        pkg.set_pairing_rlc_params(-1)
        assert pkg.pairing_rlc_params() == was
        pkg.set_pairing_rlc_params(0)
        assert pkg.pairing_rlc_params() == 64
        pkg.set_pairing_rlc_params(63)
        assert pkg.pairing_rlc_params() == 64
        pkg.set_pairing_rlc_params(1 << 20)
        assert pkg.pairing_rlc_params() == 1 << 20
        L = _raw(pkg)
        L.bn254_pairing_rlc_params.argtypes = [C.c_void_p]; L.bn254_pairing_rlc_state.argtypes = [C.c_void_p]
        assert L.bn254_pairing_rlc_params(None) == E_BAD_ARG and L.bn254_pairing_rlc_state(None) == E_BAD_ARG
        assert len(pkg.pairing_rlc_state()) == 4
        # the bound on the variable positions of an honoured shape: 0 by default, clamped to 0 .. 8, a negative value restores the default
        assert pkg.dbg_set_pairing_rlc_max_var(20) == 0 and pkg.dbg_set_pairing_rlc_max_var(-1) == 8 and pkg.dbg_set_pairing_rlc_max_var(-1) == 0
    finally:
        pkg.set_pairing_rlc_params(was)
