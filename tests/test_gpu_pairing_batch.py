"""The batch pairing product over caller-supplied pairs on the GPU (csrc/bn254_k_pairing.hip: k_pairing_load, k_miller_run_var, k_pairing_store, then the final
exponentiation and k_g16_compare): the vector classes of tests/pairing_batch_common.py, all of them mixed inside one wavefront, at batch sizes on both sides of the
wavefront and of the 256-thread block, for items of 1, 2, 3 and 8 pairs -- status bytes against the host compile of the same code (bn254_dbg_pairing_batch with device
-1) byte for byte and against the oracle's expectation, GT values against the oracle, and the three ways in (host entry, device entry on a stream of its own, probe)
against each other."""
import ctypes as C
import random

import pytest

import pairing_batch_common as V

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
_HOST = {}
_SIDE = []      # one stream beside the default one for the whole file: every stream a process creates takes a share of the runtime's few hardware queues


def _host_status(pkg, O, k):
    """the host compile's status bytes of the vectors of k pairs (once)"""
    if k not in _HOST:
        vecs = V.vectors(O, k)
        buf, _, _ = V.batch(vecs, len(vecs), k)
        _HOST[k] = pkg.dbg_pairing_batch(buf, k, n=len(vecs), device=-1, want_gt=False)[1]
    return _HOST[k]


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


@pytest.mark.parametrize("k", V.PAIR_COUNTS)
def test_kernels_against_host_compile_and_oracle(pkg, O, k):
    vecs = V.vectors(O, k)
    host = _host_status(pkg, O, k)
    assert host == bytes(v[2] for v in vecs)
    for n in SIZES:
        stride = 192 * k + (0 if n % 2 else 12)          # packed records, and records with bytes behind them (a multiple of 4: the dword loads)
        buf, exp, idx = V.batch(vecs, n, k, item_stride=stride, start=3 * n)
        if n >= 63:
            assert {V.ACCEPT, V.REJECT, V.NOT_MEMBER, V.NOT_ON_CURVE, V.NOT_IN_SUBGROUP} <= set(exp[:64])      # every class inside the first wavefront
        gt, st = pkg.dbg_pairing_batch(buf, k, n=n, item_stride=stride, device=0)
        assert st == bytes(host[j] for j in idx), (k, n, [(i, vecs[idx[i]][0], st[i], exp[i]) for i in range(n) if st[i] != exp[i]][:8])
        assert st == exp
        for i, j in enumerate(idx):
            if vecs[j][3] is not None:
                assert gt[384 * i:384 * (i + 1)] == vecs[j][3], (k, n, i, vecs[j][0])
        # the three ways in agree
        assert pkg.pairing_check_batch(buf, k, n=n, item_stride=stride, device=0) == st
        assert _device_entry(pkg, buf, k, n, stride) == st
        gt2, st2 = pkg.pairing_batch(buf, k, n=n, item_stride=stride, device=0)
        assert st2 == bytes(V.ACCEPT if s in (V.ACCEPT, V.REJECT) else s for s in st)
        for i in range(n):
            if st2[i] == V.ACCEPT:
                assert gt2[384 * i:384 * (i + 1)] == gt[384 * i:384 * (i + 1)], (k, n, i)


def test_unaligned_records(pkg, O):
    """a stride that is no multiple of 4: the loader's byte loads"""
    k = 2
    vecs = V.vectors(O, k)
    buf, exp, _ = V.batch(vecs, 70, k, item_stride=192 * k + 5)
    assert pkg.pairing_check_batch(buf, k, n=70, item_stride=192 * k + 5, device=0) == exp


def test_one_pair_equals_the_pairing_probe(pkg, O):
    rng = random.Random(0x9A2)
    n = 5
    g1s = [O.g1_mul(O.g1_gen(), rng.randrange(1, V.R)) for _ in range(n)]
    g2s = [O.g2_mul(O.g2_gen(), rng.randrange(1, V.R)) for _ in range(n)]
    L = pkg.lib()
    out = (C.c_uint8 * (384 * n))()
    assert L.bn254_dbg_pairing(b"".join(g1s), b"".join(g2s), out, C.c_size_t(n), 0) == 0
    gt, st = pkg.pairing_batch(b"".join(p + q for p, q in zip(g1s, g2s)), 1, device=0)
    assert st == bytes([V.ACCEPT] * n) and gt == bytes(out)
    assert gt[:384] == O.pairing(g1s[0], g2s[0])


def _g1_neg(p):
    return p if p == bytes(64) else p[:32] + V.be((V.P - int.from_bytes(p[32:], "big")) % V.P)


def test_groth16_restated_as_four_pairs(pkg, O):
    """32 synthetic Groth16 proofs, every second one invalid, restated as e(A, B) e(-alpha, beta) e(-L, gamma) e(-C, delta) == 1 with L and the decompressed key
    points from the oracle: ACCEPT / REJECT exactly as bn254_groth16_verify_batch answers with the key in gnark's interpretation"""
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
    assert pkg.pairing_check_batch(b"".join(items), 4, device=0) == bytes(want)
