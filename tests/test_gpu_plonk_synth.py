"""The PlonK pipeline on DISTINCT VALID proofs for several key shapes (bn254_synth_plonk): until the generator the only proofs that ever passed were the four SP1
fixtures, on one key shape.  Every status byte of the host-buffer and the device-resident entry equals the generator's expected status -- exact, and with
BN254_FLAG_RLC from the batch size at which it is honoured -- for keys with 0, 1, 2, 3 and 5 public inputs and 0, 1, 2 and 8 BSB22 commitments; samples go to the
oracle, which is what decides that the generator's proofs are valid at all.  Then the batch size at which the joint MSM rows run, a stride with junk behind the
proof, and the SP1 entry on synthetic proofs for digests of distinct public values."""
import random

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0, 10), (2, 1, 26), (3, 2, 20), (0, 0, 3), (5, 8, 28)]        # (n_public, n_qcp, log2 size)
N = 9000
OPENING_MISMATCH = 7     # BN254_ERR_OPENING_MISMATCH
PREFIXES = (1, 257, 5041, 9000)      # one lane, a partial pass, two chained passes, one pass above the 8192-proof threshold of BN254_FLAG_RLC


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


def _seed(shape):
    return 0x504C1200 + 64 * shape[0] + shape[2]


@pytest.fixture(scope="module")
def workload(pkg):
    """shape -> 9000 proofs of it, every 8th invalid, with the prepared key: generated once per shape and never changed"""
    cache = {}

    def get(shape):
        if shape not in cache:
            vk, proofs, inputs, exp = pkg.synth_plonk(_seed(shape), shape[0], shape[1], shape[2], N, invalid_every=8, threads=16)
            cache[shape] = (pkg.PreparedPlonkVk(vk), vk, proofs, inputs, exp, 808 + 96 * shape[1])
        return cache[shape]

    yield get
    for w in cache.values():
        w[0].close()


def _dev(torch_dev, pvk, proofs, inputs, n, stride, n_public, flags=0):
    torch, dev = torch_dev
    d_p = torch.frombuffer(bytearray(proofs[:n * stride]), dtype=torch.uint8).to(dev)
    d_i = torch.frombuffer(bytearray(inputs[:32 * n_public * n] or b"\0"), dtype=torch.uint8).to(dev)
    d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    pvk.verify_batch_device(d_p.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), n, proof_stride=stride, n_public=n_public, device=dev.index,
                            stream=torch.cuda.current_stream(dev).cuda_stream, flags=flags)
    return bytes(d_s.cpu().numpy().tobytes())


def _host(pvk, proofs, inputs, n, stride, n_public, flags=0):
    return pvk.verify_batch(proofs[:n * stride], inputs[:32 * n_public * n], n=n, proof_stride=stride, n_public=n_public, flags=flags)


def _oracle(O, vk, proofs, inputs, stride, plen, n_public, i):
    return O.plonk_verify(proofs[stride * i:stride * i + plen], vk, [inputs[32 * (n_public * i + j):32 * (n_public * i + j + 1)] for j in range(n_public)])


def _first_difference(got, want):
    d = [i for i in range(len(want)) if got[i] != want[i]]
    return "%d of %d status bytes differ, first at %d: got %d, expected %d" % (len(d), len(want), d[0], got[d[0]], want[d[0]]) if d else ""


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_distinct_proofs_every_shape(pkg, O, torch_dev, workload, shape):
    pvk, vk, proofs, inputs, exp, plen = workload(shape)
    n_public = shape[0]
    assert pvk.n_public == n_public and len(proofs) == N * plen
    assert len({proofs[plen * i:plen * i + 192] for i in range(N)}) == N            # distinct: no two proofs share their first commitments
    assert exp.count(bytes([pkg.ACCEPT])) > 7800
    for n in PREFIXES:
        for name, got in (("host buffers", _host(pvk, proofs, inputs, n, plen, n_public)), ("device", _dev(torch_dev, pvk, proofs, inputs, n, plen, n_public))):
            assert got == exp[:n], "%s, %d proofs: %s" % (name, n, _first_difference(got, exp[:n]))
    for name, got in (("host buffers", _host(pvk, proofs, inputs, N, plen, n_public, pkg.FLAG_RLC)), ("device", _dev(torch_dev, pvk, proofs, inputs, N, plen, n_public, pkg.FLAG_RLC))):
        assert got == exp, "%s, BN254_FLAG_RLC: %s" % (name, _first_difference(got, exp))
        assert got.count(bytes([pkg.ACCEPT])) > 7800                                     # keeps the test from passing on all-failures; not a measurement
    # a fixed sample against the oracle: the first twelve invalid proofs (every class twice) and 52 valid ones
    rng = random.Random(_seed(shape))
    sample = [8 * k + 7 for k in range(12)] + rng.sample([i for i in range(N) if i % 8 != 7], 52)
    assert len({(i // 8) % 6 for i in sample[:12]}) == 6 and sum(1 for i in sample if exp[i] == pkg.ACCEPT) >= 40
    ref = bytes(_oracle(O, vk, proofs, inputs, plen, plen, n_public, i) for i in sample)
    assert ref == bytes(exp[i] for i in sample)
    assert {exp[i] for i in sample[:12]} == {3, 2, 8} | ({7} if n_public else set()) | ({9} if shape[1] else set())


def test_joint_msm_rows_at_49200(pkg, O, torch_dev):
    """49 200 proofs in one call: the size at which the MSM launches walk joint rows; exact and BN254_FLAG_RLC"""
    shape, n = (3, 2, 20), 49200
    vk, proofs, inputs, exp = pkg.synth_plonk(_seed(shape) + 1, 3, 2, 20, n, invalid_every=8, threads=16)
    pvk = pkg.PreparedPlonkVk(vk)
    try:
        assert exp.count(bytes([pkg.ACCEPT])) == n - n // 8
        for flags in (0, pkg.FLAG_RLC):
            got = _dev(torch_dev, pvk, proofs, inputs, n, 1000, 3, flags)
            assert got == exp, "flags %d: %s" % (flags, _first_difference(got, exp))
        rng = random.Random(49200)
        sample = [8 * k + 7 for k in range(6)] + rng.sample(range(n), 26)
        assert bytes(_oracle(O, vk, proofs, inputs, 1000, 1000, 3, i) for i in sample) == bytes(exp[i] for i in sample)
    finally:
        pvk.close()


def test_stride_with_junk_behind_the_proof(pkg, torch_dev, workload):
    """records 1664 bytes apart for 1576-byte proofs, the 88 bytes between them 0xa5: the same statuses"""
    shape, n = (5, 8, 28), 1000
    pvk, vk, proofs, inputs, exp, plen = workload(shape)
    vk2, wide, in2, exp2 = pkg.synth_plonk(_seed(shape), 5, 8, 28, n, invalid_every=8, threads=16, proof_stride=1664)
    assert plen == 1576 and vk2 == vk and in2 == inputs[:160 * n] and exp2 == exp[:n]
    recs = [wide[1664 * i:1664 * i + plen] for i in range(n)]
    assert recs == [proofs[plen * i:plen * (i + 1)] for i in range(n)]
    wide = b"".join(r + b"\xa5" * 88 for r in recs)
    assert _host(pvk, wide, inputs, n, 1664, 5) == exp[:n]
    assert _dev(torch_dev, pvk, wide, inputs, n, 1664, 5) == exp[:n]


def test_sp1_plonk_from_public_values(pkg, torch_dev):
    """300 distinct (vkey hash, public values) pairs: the input rows are digests nobody chose, the proofs are made for them (bn254_synth_plonk_for_inputs)"""
    torch, dev = torch_dev
    rng = random.Random(0x5B1)
    n = 300
    vkhs = [b"\0" + rng.randbytes(31) for _ in range(n)]                            # below r, as a vkey hash is
    values = [rng.randbytes(rng.randrange(0, 200)) for _ in range(n)]
    assert len(set(zip(vkhs, values))) == n

    def rows(vals):
        return b"".join(h + pkg.sp1_public_values_digest(v) for h, v in zip(vkhs, vals))

    vk, proofs = pkg.synth_plonk_for_inputs(0x5B1, 2, 1, 26, rows(values), threads=16)
    pvk = pkg.PreparedPlonkVk(vk)

    def sp1(vals):
        pv = b"".join(vals)
        offs, acc = [0], 0
        for v in vals:
            acc += len(v)
            offs.append(acc)
        d_p = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).to(dev); d_h = torch.frombuffer(bytearray(b"".join(vkhs)), dtype=torch.uint8).to(dev)
        d_v = torch.frombuffer(bytearray(pv or b"\0"), dtype=torch.uint8).to(dev); d_o = torch.tensor(offs, dtype=torch.int64).to(dev)
        d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        pvk.verify_sp1_batch_device(d_p.data_ptr(), d_h.data_ptr(), d_v.data_ptr(), len(pv), d_o.data_ptr(), d_s.data_ptr(), n,
                                    stream=torch.cuda.current_stream(dev).cuda_stream)
        return bytes(d_s.cpu().numpy().tobytes())

    try:
        assert sp1(values) == bytes([pkg.ACCEPT] * n)
        flipped = [(bytes([v[0] ^ 1]) + v[1:] if v else b"\x01") if i % 7 == 6 else v for i, v in enumerate(values)]
        raw = _dev(torch_dev, pvk, proofs, rows(flipped), n, 904, 2)
        assert sp1(flipped) == raw
        assert raw == bytes(OPENING_MISMATCH if i % 7 == 6 else pkg.ACCEPT for i in range(n))
    finally:
        pvk.close()
