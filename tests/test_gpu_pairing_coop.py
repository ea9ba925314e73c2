"""The cooperative form of the batch pairing product on the GPU (csrc/bn254_coop12.hip::k_coop12_miller_pairs after k_pairing_load: twelve lanes per item, five items
per wavefront, the pairs' running points in the LDS slots the final exponentiation leaves free during the Miller loop), forced through
bn254_dbg_pairing_batch_form(form = 2): the vector classes of tests/pairing_batch_common.py at the wavefront boundaries of this layout -- status bytes against the
host compile (device -1) byte for byte and against the oracle's expectation, GT values against the oracle -- a batch whose wavefronts are all-decided, all-pending
and a single item, the two forms and the three entries against each other with the counters of bn254_pairing_state, the GT mode alone, and Groth16 restated as four
pairs."""
import pytest

import pairing_batch_common as V

pytestmark = pytest.mark.gpu
PAIR_COUNTS = (1, 2, 3, 5, 8)
SIZES = (1, 4, 5, 6, 11, 64, 257)          # five items per wavefront: 5, 6 and 11 are the boundaries
LANES, COOP = 1, 2
ALL_CLASSES = {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE, V.NOT_IN_SUBGROUP}
_HOST = {}
_SIDE = []      # one stream beside the default one for the whole file


def _host_status(pkg, O, k):
    """the host compile's status bytes of the vectors of k pairs (once)"""
    if k not in _HOST:
        vecs = V.vectors(O, k)
        buf, _, _ = V.batch(vecs, len(vecs), k)
        _HOST[k] = pkg.dbg_pairing_batch(buf, k, n=len(vecs), device=-1, want_gt=False)[1]
        assert _HOST[k] == bytes(v[2] for v in vecs)
    return _HOST[k]


def _items(vecs, idx, k, stride):
    return b"".join(vecs[j][1] + b"\xa5" * (stride - 192 * k) for j in idx)


def _check(pkg, O, k, vecs, idx, stride, gt, st):
    host = _host_status(pkg, O, k)
    exp = bytes(vecs[j][2] for j in idx)
    assert st == bytes(host[j] for j in idx), (k, len(idx), [(i, vecs[idx[i]][0], st[i], exp[i]) for i in range(len(idx)) if st[i] != exp[i]][:8])
    assert st == exp
    for i, j in enumerate(idx):
        if vecs[j][3] is not None:
            assert gt[384 * i:384 * (i + 1)] == vecs[j][3], (k, len(idx), i, vecs[j][0])


@pytest.mark.parametrize("k", PAIR_COUNTS)
def test_forced_cooperative_form_against_host_compile_and_oracle(pkg, O, k):
    vecs = V.vectors(O, k)
    names = [v[0] for v in vecs]
    for needle in ("g1_identity_pair0", "g2_identity_pair0", "g1_identity_pair%d" % (k - 1), "g2_identity_pair%d" % (k - 1), "g1_identity_g2_outside_pair0",
                   "g1_identity_g2_outside_pair%d" % (k - 1), "g2_outside_subgroup_pair0", "g2_outside_subgroup_pair%d" % (k - 1)):
        assert needle in names, needle
    if k >= 2:
        assert {"subgroup_pair0_curve_pair1", "curve_pair0_member_pair1", "member_pair0_curve_pair1"} <= set(names)
    assert len(vecs) <= 64       # so a batch of 64 items or more holds every vector class, at every position of a wavefront's five groups over the batch
    for n in SIZES:
        stride = 192 * k + (0 if n % 2 else 12)
        buf, exp, idx = V.batch(vecs, n, k, item_stride=stride, start=3 * n)
        if n >= 64:
            assert set(idx) == set(range(len(vecs))) and ALL_CLASSES <= set(exp)
        gt, st = pkg.dbg_pairing_batch(buf, k, n=n, item_stride=stride, device=0, form=COOP)
        _check(pkg, O, k, vecs, idx, stride, gt, st)


def test_wavefront_composition(pkg, O):
    """one wavefront whose five items the loader decides (the early return), one whose five items are all pending with an off-subgroup item among them, and a last
    wavefront of a single item (the shadow lanes 60 .. 63 and the groups past the batch are live)"""
    k = 3
    vecs = V.vectors(O, k)
    name = {v[0]: j for j, v in enumerate(vecs)}
    decided = [name[x] for x in ("g1_x_ge_p_pair0", "g2_off_curve_pair2", "g1_off_curve_pair0", "subgroup_pair0_curve_pair1", "g2_y_c0_ge_p_pair2")]
    pending = [name[x] for x in ("random0", "identity", "g1_identity_g2_outside_pair2", "g2_identity_pair0", "identity_perturbed")]
    last = [name["identity_padded"]]
    assert all(vecs[j][2] in (V.NOT_MEMBER, V.NOT_ON_CURVE) for j in decided)
    assert all(vecs[j][2] in (V.ACCEPT, V.REJECT, V.NOT_IN_SUBGROUP) for j in pending) and V.NOT_IN_SUBGROUP in [vecs[j][2] for j in pending]
    idx = decided + pending + last
    stride = 192 * k
    gt, st = pkg.dbg_pairing_batch(_items(vecs, idx, k, stride), k, n=len(idx), item_stride=stride, device=0, form=COOP)
    _check(pkg, O, k, vecs, idx, stride, gt, st)
    # ... and the same with the decided wavefront last but one, so that the early return is not the first block
    idx = pending + decided + last
    gt, st = pkg.dbg_pairing_batch(_items(vecs, idx, k, stride), k, n=len(idx), item_stride=stride, device=0, form=COOP)
    _check(pkg, O, k, vecs, idx, stride, gt, st)


def _device_entry(pkg, buf, k, n, stride):
    import torch
    dev = torch.device("cuda:0")
    d_pairs = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    pkg.pairing_reserve(n, device=0)
    torch.cuda.synchronize(dev)
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(device=dev))
    side = _SIDE[0]
    pkg.pairing_check_batch_device(d_pairs.data_ptr(), k, n, d_status.data_ptr(), item_stride=stride, device=0, stream=side.cuda_stream)
    side.synchronize()
    return bytes(d_status.cpu().numpy().tobytes())


@pytest.mark.parametrize("k", (1, 8))
def test_forms_agree(pkg, O, k):
    n = 65
    vecs = V.vectors(O, k)
    stride = 192 * k + 12
    buf, exp, idx = V.batch(vecs, n, k, item_stride=stride, start=7)
    before = pkg.pairing_params()
    try:
        pkg.set_pairing_params(4096)
        assert pkg.dbg_pairing_form(k, n) == COOP
        gt1, st1 = pkg.dbg_pairing_batch(buf, k, n=n, item_stride=stride, device=0, form=LANES)
        gt2, st2 = pkg.dbg_pairing_batch(buf, k, n=n, item_stride=stride, device=0, form=COOP)
        assert st1 == st2 == exp
        for i in range(n):
            if st1[i] in (V.ACCEPT, V.REJECT):
                assert gt1[384 * i:384 * (i + 1)] == gt2[384 * i:384 * (i + 1)], (k, i)

        def entries():
            c0, l0 = pkg.pairing_state()
            assert pkg.pairing_check_batch(buf, k, n=n, item_stride=stride, device=0) == st1
            assert _device_entry(pkg, buf, k, n, stride) == st1
            gt3, st3 = pkg.pairing_batch(buf, k, n=n, item_stride=stride, device=0)
            assert st3 == bytes(V.ACCEPT if s in (V.ACCEPT, V.REJECT) else s for s in st1)
            for i in range(n):
                if st3[i] == V.ACCEPT:
                    assert gt3[384 * i:384 * (i + 1)] == gt1[384 * i:384 * (i + 1)], (k, i)
            c1, l1 = pkg.pairing_state()
            return c1 - c0, l1 - l0

        assert entries() == (3, 0)                 # the default: three launches, all cooperative
        pkg.set_pairing_params(0)
        assert pkg.dbg_pairing_form(k, n) == LANES
        assert entries() == (0, 3)                 # the same bytes from the lane form
    finally:
        pkg.set_pairing_params(before)


def test_gt_mode_alone(pkg, O):
    """bn254_pairing_batch in the cooperative form: a pending item ends ACCEPT with the oracle's value, a decided item keeps its error and its GT bytes are left as
    the lane form leaves them"""
    k, n = 2, 7
    vecs = V.vectors(O, k)
    name = {v[0]: j for j, v in enumerate(vecs)}
    idx = [name[x] for x in ("random0", "g1_off_curve_pair0", "identity", "g2_outside_subgroup_pair1", "random1", "g1_x_ge_p_pair1", "identity_perturbed")]
    buf = _items(vecs, idx, k, 192 * k)
    before = pkg.pairing_params()
    try:
        pkg.set_pairing_params(0)
        gt_l, st_l = pkg.pairing_batch(buf, k, n=n, device=0)
        pkg.set_pairing_params(4096)
        c0, l0 = pkg.pairing_state()
        gt_c, st_c = pkg.pairing_batch(buf, k, n=n, device=0)
        assert pkg.pairing_state() == (c0 + 1, l0)
    finally:
        pkg.set_pairing_params(before)
    assert st_c == st_l == bytes(V.ACCEPT if vecs[j][2] in (V.ACCEPT, V.REJECT) else vecs[j][2] for j in idx)
    assert st_c[1] == V.NOT_ON_CURVE and st_c[3] == V.NOT_IN_SUBGROUP and st_c[5] == V.NOT_MEMBER
    for i, j in enumerate(idx):
        if st_c[i] == V.ACCEPT:
            assert gt_c[384 * i:384 * (i + 1)] == vecs[j][3], vecs[j][0]
        else:
            assert gt_c[384 * i:384 * (i + 1)] == gt_l[384 * i:384 * (i + 1)], vecs[j][0]      # not written by either form
    g1, g2 = O.g1_gen(), O.g2_gen()
    p, q = O.g1_mul(g1, 5), O.g2_mul(g2, 7)
    gt, st = pkg.dbg_pairing_batch(p + q, 1, device=0, form=COOP)
    assert st == bytes([V.REJECT]) and gt == O.pairing(p, q)


def _g1_neg(p):
    return p if p == bytes(64) else p[:32] + V.be((V.P - int.from_bytes(p[32:], "big")) % V.P)


def test_groth16_restated_as_four_pairs_cooperative(pkg, O):
    """32 synthetic Groth16 proofs, every second one invalid, restated as e(A, B) e(-alpha, beta) e(-L, gamma) e(-C, delta) == 1 (as tests/test_gpu_pairing_batch.py
    builds it) through the cooperative form: ACCEPT / REJECT exactly as bn254_groth16_verify_batch answers"""
    n, n_public = 32, 2
    vk, proofs, inputs, _ = pkg.synth_groth16(0x9A3, n_public, n, invalid_every=2, agree=True, threads=8)
    pvk = pkg.PreparedVk(vk, pkg.VK_GNARK)
    ref = pvk.verify_batch(proofs, inputs, n_public=n_public, device=0)

    def g1(b):
        st, p = O.decompress_g1(b)
        assert st == O.ACCEPT
        return p

    def g2(b):
        st, q = O.decompress_g2(b, O.MODE_GNARK)
        assert st == O.ACCEPT
        return q

    alpha, beta, gamma, delta = g1(vk[0:32]), g2(vk[64:128]), g2(vk[128:192]), g2(vk[224:288])
    nk = int.from_bytes(vk[288:292], "big")
    ks = [g1(vk[292 + 32 * i:324 + 32 * i]) for i in range(nk)]
    items, want = [], []
    for i in range(n):
        if ref[i] not in (V.ACCEPT, V.REJECT):
            continue
        pr = proofs[256 * i:256 * (i + 1)]
        L = ks[0]
        for j in range(n_public):
            x = int.from_bytes(inputs[32 * (n_public * i + j):32 * (n_public * i + j + 1)], "big") % V.R
            L = O.g1_add(L, O.g1_mul(ks[j + 1], x))
        items.append(pr[0:64] + pr[64:192] + _g1_neg(alpha) + beta + _g1_neg(L) + gamma + _g1_neg(pr[192:256]) + delta)
        want.append(ref[i])
    assert V.ACCEPT in want and V.REJECT in want and len(want) >= 8
    assert pkg.dbg_pairing_batch(b"".join(items), 4, device=0, form=COOP, want_gt=False)[1] == bytes(want)
