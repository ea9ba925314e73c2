"""The batch pairing product over caller-supplied pairs (include/bn254_verify.h, bn254_pairing_check_batch) without a GPU: the argument checks of the four entries, and
through bn254_dbg_pairing_batch(device = -1) -- the HOST compile of the loader, vm_miller_run_var and the final-exponentiation program the kernels run -- every
vector class of tests/pairing_batch_common.py against the oracle, for items of 1, 2, 3 and 8 pairs (the standard slots, the first extra slot, the last one)."""
import ctypes as C

import pytest

import pairing_batch_common as V

E_BAD_ARG = -1
NO_SUCH_DEVICE = 4097     # a call that got past the argument checks would answer BN254_E_NO_DEVICE or "device ordinal out of range" with another text, not these


def _raw(pkg):
    import sys
    return sys.modules[pkg.__name__ + ".binding"]._pairing_lib()


def test_argument_errors_touch_nothing(pkg):
    L = _raw(pkg)
    L.bn254_last_error.restype = C.c_char_p
    item = bytes(192 * 8)
    st = (C.c_uint8 * 4)(*([0xEE] * 4)); gt = (C.c_uint8 * (384 * 4))(*([0xEE] * (384 * 4)))
    stp, gtp = C.cast(st, C.c_void_p), C.cast(gt, C.c_void_p)

    def untouched():
        return bytes(st) == b"\xee" * 4 and bytes(gt) == b"\xee" * (384 * 4)

    calls = {
        "check": lambda p, s, k, n, status: L.bn254_pairing_check_batch(p, s, k, n, status, NO_SUCH_DEVICE),
        "device": lambda p, s, k, n, status: L.bn254_pairing_check_batch_device(C.cast(C.c_char_p(p), C.c_void_p) if p else None, s, k, n, status, NO_SUCH_DEVICE, None),
        "gt": lambda p, s, k, n, status: L.bn254_pairing_batch(p, s, k, n, gtp, status, NO_SUCH_DEVICE),
        "probe": lambda p, s, k, n, status: L.bn254_dbg_pairing_batch(p, s, k, n, gtp, status, NO_SUCH_DEVICE),
    }
    for name, call in calls.items():
        assert call(None, 192, 1, 1, stp) == E_BAD_ARG and untouched(), name                 # null pairs with n > 0
        assert call(item, 192, 1, 1, None) == E_BAD_ARG and untouched(), name                # null status with n > 0
        assert call(item, 192, 0, 1, stp) == E_BAD_ARG and untouched(), name                 # n_pairs 0
        assert call(item, 192 * 9, 9, 1, stp) == E_BAD_ARG and untouched(), name             # n_pairs above 8
        assert call(item, 191, 1, 1, stp) == E_BAD_ARG and untouched(), name                 # short stride
        assert call(item, 192 * 8 - 1, 8, 1, stp) == E_BAD_ARG and untouched(), name
        assert call(item, 192 * 3, 3, 0, stp) == 0 and untouched(), name                     # n == 0
        assert call(None, 192, 1, 0, None) == 0 and untouched(), name
        # an argument set that passes the checks reaches the device check, and says so
        rc = call(item, 192, 1, 1, stp)
        assert rc in (-1, -2) and rc != 0 and untouched(), name
        assert b"device" in L.bn254_last_error().lower(), name
    assert L.bn254_pairing_batch(item, 192, 1, 1, None, stp, NO_SUCH_DEVICE) == E_BAD_ARG and untouched()    # null out_gt with n > 0
    assert L.bn254_dbg_pairing_batch(item, 192, 1, 1, gtp, stp, -2) == E_BAD_ARG and untouched()


@pytest.mark.parametrize("k", V.PAIR_COUNTS)
def test_host_compile_against_the_oracle(pkg, O, k):
    """every vector class for items of k pairs, one probe call over all of them (so the items also differ inside one call), at a stride with padding: status bytes
    and, where the item reaches the pairing, the 384 bytes of the GT value"""
    vecs = V.vectors(O, k)
    names = [v[0] for v in vecs]
    for needle in ("random0", "g1_identity_pair0", "g2_identity_pair%d" % (k - 1), "g1_x_ge_p_pair0", "g2_y_c0_ge_p_pair%d" % (k - 1), "g1_off_curve_pair%d" % (k - 1),
                   "g2_off_curve_pair0", "g2_outside_subgroup_pair0", "g2_outside_subgroup_pair%d" % (k - 1)):
        assert needle in names, needle
    if k >= 2:
        assert {"identity", "identity_padded", "identity_perturbed", "subgroup_pair0_curve_pair1"} <= set(names)
    stride = 192 * k + 7
    buf, exp, _ = V.batch(vecs, len(vecs), k, item_stride=stride)
    gt, st = pkg.dbg_pairing_batch(buf, k, n=len(vecs), item_stride=stride, device=-1)
    for i, (name, _, status, want) in enumerate(vecs):
        assert st[i] == status, (k, name, st[i], status)
        if want is not None:
            assert gt[384 * i:384 * (i + 1)] == want, (k, name)
    assert st == exp
    assert {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE, V.NOT_IN_SUBGROUP} <= set(st)
    # the same items without a GT buffer: same status bytes
    none, st2 = pkg.dbg_pairing_batch(buf, k, n=len(vecs), item_stride=stride, device=-1, want_gt=False)
    assert none is None and st2 == st


def test_host_compile_with_the_loop_cut_into_runs(pkg, O):
    """BN254_MILLER_RUN_STEPS (read once per process, so a child process): the Miller loop as runs of 11 steps -- f stored and loaded between them, the r-torsion
    tests in the last run -- gives the GT values and status bytes of the one-run loop, which the test above holds to the oracle"""
    import os
    import subprocess
    import sys
    k = 3
    vecs = V.vectors(O, k)
    buf, exp, _ = V.batch(vecs, len(vecs), k)
    gt, st = pkg.dbg_pairing_batch(buf, k, n=len(vecs), device=-1)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = ("import sys, importlib; sys.path.insert(0, %r); pkg = importlib.import_module('snark-bn254-verifier_amd'); buf = sys.stdin.buffer.read(); "
             "gt, st = pkg.dbg_pairing_batch(buf, %d, device=-1); sys.stdout.buffer.write(st + gt)" % (root, k))
    r = subprocess.run([sys.executable, "-c", child], input=buf, capture_output=True, env=dict(os.environ, BN254_MILLER_RUN_STEPS="11"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert st == exp and r.stdout[:len(vecs)] == st
    for i, v in enumerate(vecs):
        if v[3] is not None:
            assert r.stdout[len(vecs) + 384 * i:len(vecs) + 384 * (i + 1)] == gt[384 * i:384 * (i + 1)] == v[3], v[0]


def test_pass_plan_fits_the_reservation(pkg):
    """every pass of the host entries fits the workspace a reservation of the same n allocates, no pass is above 2^18 items or 48 MB of pinned records"""
    for k in range(1, 9):
        for n in (1, 255, 4096, 32768, 32769, 2 ** 18, 2 ** 18 + 1, 10 ** 6, 2 ** 22):
            p = pkg.dbg_pairing_plan(k, n)
            assert 1 <= p["pass_items"] <= p["ws_items"] <= 2 ** 18 and p["ws_items"] == min(n, 2 ** 18)
            assert p["pinned_bytes"] == p["pass_items"] * 192 * k <= 48 << 20
            assert (p["passes"] - 1) * p["pass_items"] < n <= p["passes"] * p["pass_items"]
