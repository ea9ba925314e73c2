"""Pairing batches with shared, prepared G2 points on the GPU (csrc/bn254_k_pairing.hip: k_pairing_load_shared, k_miller_run_mix in both instantiations, then the
existing tails; small launches: k_coop12_miller_pairs after the shared loader): the vector classes of tests/pairing_shared_common.py, all of them inside one wavefront,
at batch sizes on both sides of the wavefront and of the 256-thread block, both forms forced through the probe -- status bytes and GT values against the host compile
of the same code byte for byte and against the oracle; the three ways in against each other; a corrupted record through the device entry; Groth16 proofs restated with
the key's three G2 points prepared; a KZG-shaped batch; the counters of bn254_pairing_state."""
import random
import struct

import pytest

import pairing_batch_common as V
import pairing_shared_common as S

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)           # a wavefront is 64 lanes, a block 256: the partial wavefront, the full one, the second one, the second block's first lane
LANES, COOP = 1, 2
_HOST = {}
_PREP = {}
_SIDE = []      # one stream beside the default one for the whole file (tests/test_gpu_pairing_batch.py says why)


def _prepared(pkg, O, k, mask):
    if (k, mask) not in _PREP:
        shared, _ = S.vectors(O, k, mask)
        recs = [pkg.g2_prepare(shared[j]) for j in sorted(shared)]
        assert all(st == V.ACCEPT for st, _ in recs)
        _PREP[(k, mask)] = b"".join(r for _, r in recs)
    return _PREP[(k, mask)]


def _host(pkg, O, k, mask):
    """the host compile's (GT values, status bytes) of the shape's vectors (once)"""
    if (k, mask) not in _HOST:
        _, vecs = S.vectors(O, k, mask)
        packed, _, _, _ = S.batch(vecs, len(vecs), k, mask)
        _HOST[(k, mask)] = pkg.dbg_pairing_batch_shared(packed, k, mask, _prepared(pkg, O, k, mask), n=len(vecs), device=-1)
    return _HOST[(k, mask)]


def _device_entry(pkg, buf, k, mask, prep, n, stride):
    import torch
    dev = torch.device("cuda:0")
    d_items = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    d_prep = torch.frombuffer(bytearray(prep), dtype=torch.uint8).to(dev)
    assert d_prep.data_ptr() % 4 == 0
    d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    pkg.pairing_reserve(n, device=0)
    torch.cuda.synchronize(dev)
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(device=dev))
    side = _SIDE[0]
    pkg.pairing_check_batch_shared_device(d_items.data_ptr(), k, mask, d_prep.data_ptr(), n, d_status.data_ptr(), item_stride=stride, device=0, stream=side.cuda_stream)
    side.synchronize()
    return bytes(d_status.cpu().numpy().tobytes())


@pytest.mark.parametrize("k,mask", S.SHAPES)
def test_kernels_against_host_compile_and_oracle(pkg, O, k, mask):
    _, vecs = S.vectors(O, k, mask)
    prep = _prepared(pkg, O, k, mask)
    host_gt, host_st = _host(pkg, O, k, mask)
    assert host_st == bytes(v[3] for v in vecs)
    before = pkg.pairing_params()
    try:
        for n in SIZES:
            stride = S.packed_len(k, mask) + (0 if n % 2 else 12)
            buf, _, exp, idx = S.batch(vecs, n, k, mask, item_stride=stride, start=3 * n)
            if n >= 63:
                assert set(exp[:64]) == S.statuses_of(k, mask)                      # every class the shape can produce inside the first wavefront
            for form in (LANES, COOP):
                c0, l0 = pkg.pairing_state()
                gt, st = pkg.dbg_pairing_batch_shared(buf, k, mask, prep, n=n, item_stride=stride, device=0, form=form)
                c1, l1 = pkg.pairing_state()
                assert (c1 - c0, l1 - l0) == ((1, 0) if form == COOP else (0, 1)), (k, mask, n, form)
                assert st == bytes(host_st[j] for j in idx), (k, mask, n, form, [(i, vecs[idx[i]][0], st[i], exp[i]) for i in range(n) if st[i] != exp[i]][:8])
                assert st == exp
                for i, j in enumerate(idx):
                    if vecs[j][4] is not None:
                        assert gt[384 * i:384 * (i + 1)] == vecs[j][4] == host_gt[384 * j:384 * (j + 1)], (k, mask, n, form, i, vecs[j][0])
            # the three ways in agree, in the form the plan chooses (cooperative at these sizes) and in the lane form
            for coop_max in (before, 0):
                pkg.set_pairing_params(coop_max)
                if n in (1, 65, 257) or coop_max == 0:
                    assert pkg.pairing_check_batch_shared(buf, k, mask, prep, n=n, item_stride=stride, device=0) == st
                    assert _device_entry(pkg, buf, k, mask, prep, n, stride) == st
                    gt2, st2 = pkg.pairing_batch_shared(buf, k, mask, prep, n=n, item_stride=stride, device=0)
                    assert st2 == bytes(V.ACCEPT if s in (V.ACCEPT, V.REJECT) else s for s in st)
                    for i in range(n):
                        if st2[i] == V.ACCEPT:
                            assert gt2[384 * i:384 * (i + 1)] == gt[384 * i:384 * (i + 1)], (k, mask, n, i)
            pkg.set_pairing_params(before)
    finally:
        pkg.set_pairing_params(before)


def test_unaligned_items(pkg, O):
    """a stride that is no multiple of 4: the loader's byte loads on the packed record"""
    k, mask = 4, 0b1110
    _, vecs = S.vectors(O, k, mask)
    stride = S.packed_len(k, mask) + 5
    buf, _, exp, _ = S.batch(vecs, 70, k, mask, item_stride=stride)
    assert pkg.dbg_pairing_batch_shared(buf, k, mask, _prepared(pkg, O, k, mask), n=70, item_stride=stride, device=0, form=LANES, want_gt=False)[1] == exp


def test_corrupted_record_through_the_device_entry(pkg, O):
    """the device entry cannot read the record on the host: its loader kernel finds the wrong magic word (or version) of ANY record, every item ends MALFORMED, no run
    kernel has a pending item, and the next call with the sound records answers right"""
    k, mask = 4, 0b1110
    _, vecs = S.vectors(O, k, mask)
    prep = _prepared(pkg, O, k, mask)
    L = pkg.G2_PREPARED_LEN
    before = pkg.pairing_params()
    try:
        for coop_max, n in ((before, 65), (0, 65), (0, 257)):
            pkg.set_pairing_params(coop_max)
            buf, _, exp, _ = S.batch(vecs, n, k, mask)
            for word, value in ((0, 0x50324743), (1, 2)):
                bad = bytearray(prep)
                struct.pack_into("<I", bad, 2 * L + 4 * word, value)             # the LAST record
                assert _device_entry(pkg, buf, k, mask, bytes(bad), n, S.packed_len(k, mask)) == bytes([pkg.ERR_MALFORMED]) * n
            assert _device_entry(pkg, buf, k, mask, prep, n, S.packed_len(k, mask)) == exp
    finally:
        pkg.set_pairing_params(before)


def _g1_neg(p):
    return p if p == bytes(64) else p[:32] + V.be((V.P - int.from_bytes(p[32:], "big")) % V.P)


def test_groth16_restated_with_the_key_prepared(pkg, O):
    """the 32 synthetic Groth16 proofs of tests/test_gpu_pairing_batch.py::test_groth16_restated_as_four_pairs as e(A, B) e(-alpha, beta) e(-L, gamma) e(-C, delta) == 1
    with beta, gamma, delta prepared (mask 0b1110): the bytes of bn254_groth16_verify_batch with the key in gnark's interpretation, in both forms"""
    n, n_public = 32, 2
    vk, proofs, inputs, _ = pkg.synth_groth16(0x9A3, n_public, n, invalid_every=2, agree=True, threads=8)
    pvk = pkg.PreparedVk(vk, pkg.VK_GNARK)
    ref = pvk.verify_batch(proofs, inputs, n_public=n_public, device=0)
    assert len(ref) == n

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
    assert nk == n_public + 1
    ks = [g1(vk[292 + 32 * i:324 + 32 * i]) for i in range(nk)]
    recs = []
    for q in (beta, gamma, delta):
        st, rec = pkg.g2_prepare(q)
        assert st == V.ACCEPT
        recs.append(rec)
    items, want = [], []
    for i in range(n):
        if ref[i] not in (V.ACCEPT, V.REJECT):
            continue
        pr = proofs[256 * i:256 * (i + 1)]
        L = ks[0]
        for j in range(n_public):
            x = int.from_bytes(inputs[32 * (n_public * i + j):32 * (n_public * i + j + 1)], "big") % V.R
            L = O.g1_add(L, O.g1_mul(ks[j + 1], x))
        items.append(pr[0:64] + pr[64:192] + _g1_neg(alpha) + _g1_neg(L) + _g1_neg(pr[192:256]))
        want.append(ref[i])
    assert V.ACCEPT in want and V.REJECT in want and len(want) >= 8
    buf = b"".join(items)
    assert len(items[0]) == S.packed_len(4, 0b1110)
    assert pkg.pairing_check_batch_shared(buf, 4, 0b1110, recs, device=0) == bytes(want)
    for form in (LANES, COOP):
        assert pkg.dbg_pairing_batch_shared(buf, 4, 0b1110, recs, device=0, form=form, want_gt=False)[1] == bytes(want)


def test_kzg_shaped_batch(pkg, O):
    """e(C - v G1 + z W, [1]_2) e(-W, [tau]_2) == 1 for a commitment C = p(tau) G1 to a polynomial with p(z) = v, W = (p(tau) - v) / (tau - z) G1: two pairs, both G2
    points constants of the setup (mask 0b11).  Scalars only: the verdict follows from the integers -- every other opening claims v + 1"""
    rng = random.Random(0x4B5A)
    g1, g2 = O.g1_gen(), O.g2_gen()
    tau = rng.randrange(2, V.R)
    tau_g2 = O.g2_mul(g2, tau)
    recs = []
    for q in (g2, tau_g2):
        st, rec = pkg.g2_prepare(q)
        assert st == V.ACCEPT
        recs.append(rec)
    items, want = [], []
    for i in range(70):
        coeffs = [rng.randrange(V.R) for _ in range(4)]
        z = rng.randrange(V.R)
        at = lambda x: sum(c * pow(x, e, V.R) for e, c in enumerate(coeffs)) % V.R
        v, ptau = at(z), at(tau)
        w = (ptau - v) * pow((tau - z) % V.R, -1, V.R) % V.R
        claimed = (v + (i & 1)) % V.R
        p0 = (ptau - claimed + z * w) % V.R
        items.append((bytes(64) if p0 == 0 else O.g1_mul(g1, p0)) + _g1_neg(O.g1_mul(g1, w)))
        # sum a_j b_j = (ptau - claimed + z w) - w tau = v - claimed
        want.append(V.ACCEPT if claimed == v else V.REJECT)
        assert (O.pairing(items[-1], g2 + tau_g2) == V.GT_ONE) == (claimed == v)          # the oracle's verdict on the expanded pairs
    buf = b"".join(items)
    for form in (LANES, COOP):
        assert pkg.dbg_pairing_batch_shared(buf, 2, 0b11, recs, device=0, form=form, want_gt=False)[1] == bytes(want)
    assert pkg.pairing_check_batch_shared(buf, 2, 0b11, recs, device=0) == bytes(want)
