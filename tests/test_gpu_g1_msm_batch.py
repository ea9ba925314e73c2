"""Batch G1 multi-scalar multiplication on the GPU (include/bn254_verify.h: bn254_g1_bases_prepare, bn254_g1_msm_batch, _device, bn254_g1_msm_reserve; the new kernels
k_g1_msm_load and k_g1_msm_store around k_g1_msm_rows / k_g1_sum_affine): the vector classes of tests/g1_msm_common.py through the probe on the device in the split, the
unsplit and the joint form and through the public host entry at batch sizes on both sides of the wavefront, against the oracle and against the host compile of the same
code, byte for byte; the enqueue-only entry on device-resident items; sizes that cross the plan's hand-overs and a pass; shared bases with an identity base and two
handles; and the user this is built for -- the public-input sums of Groth16 proofs fed, device to device, into the shared-G2 pairing check."""
import random

import pytest

import g1_msm_common as M
import pairing_batch_common as V
import pyref_groth16 as PR
import test_gpu_pairing_batch as _PB
from test_g1_msm_cpu import FORMS, _check

pytestmark = pytest.mark.gpu
E_BAD_ARG = -1
SIZES = (1, 63, 64, 65, 130)
_SIDE = _PB._SIDE      # THE stream beside the default one, shared with the pairing tests (tests/test_gpu_pairing_batch.py)
_HOST = {}


def _side(dev):
    import torch
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(device=dev))
    return _SIDE[0]


def _host130(pkg, O, shape):
    """the host compile's answer for 130 items cycling through the shape's vectors, once, itself held to the oracle"""
    if shape not in _HOST:
        _, bpts, vecs = M.vectors(O, shape)
        ilen = pkg.g1_msm_item_len(*shape)
        buf, mem = M.batch(vecs, 130, ilen)
        r = pkg.dbg_g1_msm_batch(buf, *shape, base_points=bpts, device=-1)
        assert (r["out"], r["status"]) == M.expected(O, mem)
        _HOST[shape] = (buf, mem, r["out"], r["status"])
    return _HOST[shape]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("shape", M.SHAPES, ids=["%d-%d-%d" % s for s in M.SHAPES])
def test_kernels_against_host_compile_and_oracle(pkg, O, shape, form):
    """every vector class of the shape through the probe on the device with the form forced: status bytes and sums are the oracle's (inside _check) and, byte for byte,
    those of the host compile of the same loader, rows, row sum and store; then with BN254_FLAG_STRICT_SCALARS at a stride that is no multiple of 4 (the byte path)"""
    dev = _check(pkg, O, shape, False, form, 0, device=0)
    host = _check(pkg, O, shape, False, form, 0, device=-1)
    assert dev["out"] == host["out"] and dev["status"] == host["status"] and (dev["rows"], dev["form"], dev["chain"]) == (host["rows"], host["form"], host["chain"])
    _check(pkg, O, shape, True, form, 5, device=0)


@pytest.mark.parametrize("shape", M.SHAPES, ids=["%d-%d-%d" % s for s in M.SHAPES])
def test_host_entry_at_sizes_around_a_wavefront(pkg, O, shape):
    """bn254_g1_msm_batch at n = 1, 63, 64, 65 and 130, packed and padded: the oracle's bytes and the host compile's, and more than half of every batch from 63 items on
    is summed to a point other than the identity"""
    buf, mem, h_out, h_st = _host130(pkg, O, shape)
    bs, bpts, vecs = M.vectors(O, shape)
    ilen = pkg.g1_msm_item_len(*shape)
    st, bases = pkg.g1_bases_prepare(bpts, device=0) if shape[2] else (M.ACCEPT, None)
    assert st == M.ACCEPT and (bases is None or len(bases) == shape[2])
    try:
        for n in SIZES:
            out, status = pkg.g1_msm_batch(buf[:ilen * n], *shape, bases=bases, device=0)
            assert status == h_st[:n] and out == h_out[:64 * n], (shape, n)
            assert (out, status) == M.expected(O, mem[:n])
            if n >= 63:
                assert M.summed_share(O, mem[:n]) > 0.5
        pbuf, pmem = M.batch(vecs, 65, ilen, ilen + 7)
        for strict in (False, True):
            got = pkg.g1_msm_batch(pbuf, *shape, bases=bases, n=65, stride=ilen + 7, device=0, flags=pkg.FLAG_STRICT_SCALARS if strict else 0)
            assert got == M.expected(O, pmem, strict), (shape, strict)
            assert M.summed_share(O, pmem, strict) > 0.5
    finally:
        if bases is not None:
            bases.close()


@pytest.mark.parametrize("shape", ((1, 0, 0), (0, 2, 0), (3, 1, 2)), ids=("ecmul", "ecadd", "3-1-2"))
def test_device_entry_writes_exactly_its_bytes_and_allocates_nothing_after_a_reserve(pkg, O, shape):
    """device-resident items, out and status prefilled with 0xEE and 64 guard bytes behind each: exactly 64 n and n bytes are written; after bn254_g1_msm_reserve of the
    same shape the call makes no allocation (the entry's own counter), at the reservation and below it; above it the buffers may grow and the answer is the same"""
    import torch
    dev = torch.device("cuda:0")
    buf, mem, h_out, h_st = _host130(pkg, O, shape)
    _, bpts, _ = M.vectors(O, shape)
    ilen = pkg.g1_msm_item_len(*shape)
    st, bases = pkg.g1_bases_prepare(bpts, device=0) if shape[2] else (M.ACCEPT, None)
    assert st == M.ACCEPT
    side = _side(dev)
    try:
        d_items = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
        pkg.g1_msm_reserve(100, *shape, device=0)
        for n in (100, 37, 130):
            d_out = torch.full((64 * n + 64,), 0xEE, dtype=torch.uint8, device=dev)
            d_status = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            before = pkg.dbg_g1_msm_batch_state(*shape)["allocs"]
            pkg.g1_msm_batch_device(d_items.data_ptr(), *shape, n, d_out.data_ptr(), d_status.data_ptr(), bases=bases, device=0, stream=side.cuda_stream)
            after = pkg.dbg_g1_msm_batch_state(*shape)["allocs"]
            side.synchronize()
            assert n > 100 or after == before, (n, before, after)
            out, status = bytes(d_out.cpu().numpy().tobytes()), bytes(d_status.cpu().numpy().tobytes())
            assert out == h_out[:64 * n] + b"\xee" * 64 and status == h_st[:n] + b"\xee" * 64, (shape, n)
        # an odd address and a stride that is no multiple of 4: the byte paths of the loader and of the store
        n, stride = 66, ilen + 3
        pbuf, pmem = M.batch(M.vectors(O, shape)[2], n, ilen, stride)
        d_p = torch.frombuffer(bytearray(b"\x00" + pbuf), dtype=torch.uint8).to(dev)
        d_out = torch.full((64 * n + 65,), 0xEE, dtype=torch.uint8, device=dev)
        d_status = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pkg.g1_msm_batch_device(d_p.data_ptr() + 1, *shape, n, d_out.data_ptr() + 1, d_status.data_ptr(), bases=bases, stride=stride, device=0, stream=side.cuda_stream,
                                flags=pkg.FLAG_STRICT_SCALARS)
        side.synchronize()
        want_out, want_st = M.expected(O, pmem, True)
        assert bytes(d_out.cpu().numpy().tobytes()) == b"\xee" + want_out + b"\xee" * 64 and bytes(d_status.cpu().numpy().tobytes()) == want_st + b"\xee" * 64
    finally:
        if bases is not None:
            bases.close()


def _cyclic(pool, n, ilen, step):
    idx = [(i * step) % len(pool) for i in range(n)]
    return b"".join(pool[j].rec for j in idx), idx


def _expect_cyclic(O, pool, idx, strict=False):
    outs = [M.expected(O, [x], strict) for x in pool]
    return b"".join(outs[j][0] for j in idx), bytes(outs[j][1][0] for j in idx)


@pytest.mark.parametrize("n", (16384, 16448))
def test_split_to_unsplit_hand_over(pkg, O, n):
    """shape (2, 0, 0) on both sides of the size at which a launch stops splitting its variable terms over two rows (4 n_pad lanes against the budget of 65 536): items
    drawn cyclically, 3 apart, from 257 vectors the oracle computed once, so every wavefront holds valid items, scalars above r and items with a point off the curve"""
    shape = (2, 0, 0)
    assert pkg.dbg_g1_msm_batch_plan(*shape, 16384) == 4 and pkg.dbg_g1_msm_batch_plan(*shape, 16448) == 2
    _, _, pool = M.pool257(O, shape)
    buf, idx = _cyclic(pool, n, 192, 3)
    out, status = pkg.g1_msm_batch(buf, *shape, n=n, device=0)
    want = _expect_cyclic(O, pool, idx)
    assert status == want[1] and out == want[0]
    assert status.count(bytes([M.ACCEPT])) > n // 2 and M.NOT_ON_CURVE in status


def test_one_pass_and_65_items(pkg, O):
    """shape (1, 0, 0) at the items of a pass and 65 more: the second pass starts where the first ended, out and status of both are in place"""
    shape = (1, 0, 0)
    n = pkg.dbg_g1_msm_batch_state(*shape)["pass_items"] + 65
    _, _, pool = M.pool257(O, shape)
    buf, idx = _cyclic(pool, n, 96, 5)
    out, status = pkg.g1_msm_batch(buf, *shape, n=n, device=0, flags=pkg.FLAG_STRICT_SCALARS)
    want = _expect_cyclic(O, pool, idx, True)
    assert status == want[1] and out == want[0]
    assert {M.ACCEPT, M.NOT_MEMBER, M.NOT_ON_CURVE} == set(status) and status.count(bytes([M.ACCEPT])) > n // 2


def test_shared_bases_two_handles(pkg, O):
    """16 bases with an identity base among them, shapes (0, 0, 16) and (4, 1, 16); a second handle of other points alive at the same time; the limits of a handle are
    argument errors before a device is touched; one handle freed, the other still answers"""
    bs, bpts = M.bases(O, 16)
    assert bs.count(0) == 1
    st, a = pkg.g1_bases_prepare(bpts, device=0)
    assert st == M.ACCEPT and len(a) == 16
    rng = random.Random(0x2BA5E5)
    bs2 = [rng.randrange(2, M.R) for _ in range(3)]
    st, b = pkg.g1_bases_prepare(b"".join(M.g1_of(O, x) for x in bs2), device=0)
    assert st == M.ACCEPT and len(b) == 3
    pool = M.point_pool(O)

    def items(shape, base_scalars, n):
        v, u, s = shape
        recs, want = [], []
        for i in range(n):
            var = [(rng.choice(pool), rng.randrange(2 ** 256)) for _ in range(v)]
            unit = [rng.choice(pool) for _ in range(u)]
            shared = [rng.randrange(2 ** 256) if i % 3 else (0, 1, M.R - 1)[i % 9 // 3] for _ in range(s)]
            recs.append(M.encode(O, var, unit, shared))
            want.append(M.g1_of(O, sum(p * k for p, k in var) + sum(unit) + sum(c * q for c, q in zip(shared, base_scalars))))
        return b"".join(recs), b"".join(want)

    try:
        for shape in ((0, 0, 16), (4, 1, 16)):
            buf, want = items(shape, bs, 70)
            out, status = pkg.g1_msm_batch(buf, *shape, bases=a, device=0)
            assert status == bytes([M.ACCEPT] * 70) and out == want, shape
            assert out.count(bytes(64)) < 35
        buf3, want3 = items((1, 0, 3), bs2, 65)
        assert pkg.g1_msm_batch(buf3, 1, 0, 3, bases=b, device=0) == (want3, bytes([M.ACCEPT] * 65))
        # fewer shared terms than the handle has bases: the first ones
        buf2, want2 = items((0, 1, 2), bs2, 10)
        assert pkg.g1_msm_batch(buf2, 0, 1, 2, bases=b, device=0) == (want2, bytes([M.ACCEPT] * 10))
        for bad in (lambda: pkg.g1_msm_batch(bytes(32 * 4 * 2), 0, 0, 4, bases=b, device=0),          # n_shared above the handle's count
                    lambda: pkg.g1_msm_batch(buf3, 1, 0, 3, bases=b, device=1),                         # the handle is device 0's
                    lambda: pkg.g1_msm_batch(buf3, 1, 0, 3, bases=b, device=0, flags=pkg.FLAG_RLC)):
            with pytest.raises(pkg.Bn254Error) as e:
                bad()
            assert e.value.code == E_BAD_ARG
        a.close()
        assert pkg.g1_msm_batch(buf3, 1, 0, 3, bases=b, device=0) == (want3, bytes([M.ACCEPT] * 65))
    finally:
        a.close(); b.close()


def _enc_g1(p):
    return bytes(64) if p is None else V.be(p[0]) + V.be(p[1])


def _enc_g2(q):
    return bytes(128) if q is None else V.be(q[0][1]) + V.be(q[0][0]) + V.be(q[1][1]) + V.be(q[1][0])


def _neg_bytes(p):
    """-P for a point of 64 bytes; a point the loader will refuse anyway (a coordinate >= p) and the identity stay as they are"""
    y = int.from_bytes(p[32:], "big")
    return p if p == bytes(64) or y >= V.P or y == 0 else p[:32] + V.be(V.P - y)


def test_groth16_public_input_sums_feed_the_shared_pairing_check(pkg, O):
    """130 synthetic Groth16 proofs of a 2-input key, every 8th invalid.  The key's points come from the Python reference's parser in gnark mode; -IC_1, -IC_2 are shared
    bases, -IC_0 a unit term, so the device sums -L_i = -(IC_0 + x_1 IC_1 + x_2 IC_2); they go, device to device, into the restated item e(A, B) e(-alpha, beta)
    e(-L, gamma) e(-C, delta) == 1 with beta, gamma, delta prepared: the status bytes are those of bn254_groth16_verify_batch with BN254_VK_GNARK on the same proofs"""
    import torch
    dev = torch.device("cuda:0")
    n, n_public = 130, 2
    vk, proofs, inputs, _ = pkg.synth_groth16(0x6D5A, n_public, n, invalid_every=8, agree=True, threads=8)
    ref = pkg.PreparedVk(vk, pkg.VK_GNARK).verify_batch(proofs, inputs, n_public=n_public, device=0)
    assert len(ref) == n and ref.count(bytes([V.ACCEPT])) >= n // 2 and ref.count(bytes([V.ACCEPT])) < n
    key = PR.load_vk(vk, PR.MODE_GNARK)
    assert len(key["k"]) == n_public + 1
    neg_ic = [_enc_g1(PR.G1C.negate(p)) for p in key["k"]]
    recs = []
    for q in (PR.G2C.negate(key["beta2"]), key["gamma2"], key["delta2"]):      # load_vk holds beta negated
        st, rec = pkg.g2_prepare(_enc_g2(q))
        assert st == V.ACCEPT
        recs.append(rec)
    st, bases = pkg.g1_bases_prepare(neg_ic[1] + neg_ic[2], device=0)
    assert st == M.ACCEPT
    try:
        # MSM items: the unit term -IC_0, then the proof's two public inputs as they stand
        msm_items = b"".join(neg_ic[0] + inputs[64 * i:64 * i + 64] for i in range(n))
        neg_alpha = _enc_g1(PR.G1C.negate(key["alpha"]))
        pair_items = b"".join(proofs[256 * i:256 * i + 192] + neg_alpha + bytes(64) + _neg_bytes(proofs[256 * i + 192:256 * i + 256]) for i in range(n))
        d_msm = torch.frombuffer(bytearray(msm_items), dtype=torch.uint8).to(dev)
        d_pairs = torch.frombuffer(bytearray(pair_items), dtype=torch.uint8).to(dev).view(n, 384)
        d_recs = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(dev)
        d_sum = torch.full((n, 64), 0xEE, dtype=torch.uint8, device=dev)
        d_st_msm = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        assert d_recs.data_ptr() % 4 == 0
        pkg.g1_msm_reserve(n, 0, 1, 2, device=0)
        pkg.pairing_reserve(n, device=0)
        torch.cuda.synchronize(dev)
        side = _side(dev)
        with torch.cuda.stream(side):
            pkg.g1_msm_batch_device(d_msm.data_ptr(), 0, 1, 2, n, d_sum.data_ptr(), d_st_msm.data_ptr(), bases=bases, device=0, stream=side.cuda_stream)
            d_pairs[:, 256:320] = d_sum
            pkg.pairing_check_batch_shared_device(d_pairs.data_ptr(), 4, 0b1110, d_recs.data_ptr(), n, d_status.data_ptr(), device=0, stream=side.cuda_stream)
        side.synchronize()
        assert bytes(d_st_msm.cpu().numpy().tobytes()) == bytes([M.ACCEPT] * n)
        # the sums themselves, against the oracle
        sums = bytes(d_sum.cpu().numpy().tobytes())
        ic = [_enc_g1(p) for p in key["k"]]
        for i in (0, 7, 64, 129):
            x1, x2 = (int.from_bytes(inputs[64 * i + 32 * j:64 * i + 32 * j + 32], "big") % V.R for j in range(2))
            L = O.g1_add(ic[0], O.g1_add(O.g1_mul(ic[1], x1) if x1 else bytes(64), O.g1_mul(ic[2], x2) if x2 else bytes(64)))
            assert sums[64 * i:64 * i + 64] == _neg_bytes(L), i
        assert bytes(d_status.cpu().numpy().tobytes()) == ref
    finally:
        bases.close()
