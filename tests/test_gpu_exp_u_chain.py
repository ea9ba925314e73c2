"""Every caller of the exponentiation by u (bn254_vm.h::vm_exp_u, the addition-subtraction chain BN_U_CHAIN_*) on the smallest batches at which its
kernels can go wrong: the lane kernels on 65 proofs (two wavefronts, the second with one live lane), the cooperative Groth16 kernel on 6 proofs (a
wavefront holds five twelve-lane groups: one full wavefront and one with a single group) and the PlonK pairing check on 5 proofs.  The batches come
from the synthetic generators with every failure class present; every status byte is compared with the generator's expectation and with the oracle."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16_SEED, PLONK_SEED = 0xE0B50016, 0xE0B50B10
PLONK_SHAPE = (2, 1, 12)          # public inputs, BSB22 commitments, log2 rows: the shape with all six failure classes of the generator
FINAL_EXP_RUNS, FINAL_EXP_PRODUCTS = 36, 54      # k_f12_cyclo_sqr_n and k_f12_mul (the last one carries the verdict) launches per sub-batch


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


def _g16_device(torch_dev, pvk, proofs, inputs, n):
    torch, dev = torch_dev
    d_p = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).to(dev)
    d_i = torch.frombuffer(bytearray(inputs), dtype=torch.uint8).to(dev)
    d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    pvk.verify_batch_device(d_p.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), n, 256, 2, 0, stream.cuda_stream)
    stream.synchronize()
    return bytes(d_s.cpu().numpy().tobytes())


# the child of test_lane_kernels_65_proofs: BN254_COOP=0 is read once, when the first batch is launched, so the lane form of a small batch needs a process of its own
_LANE_CHILD = r"""
import importlib, json, sys
import torch
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module("snark-bn254-verifier_amd")
seed, n = int(sys.argv[2]), int(sys.argv[3])
vk, proofs, inputs, exp = pkg.synth_groth16(seed, 2, n, invalid_every=8, agree=True, threads=8)
pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
dev = torch.device("cuda:0")
d_p = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).to(dev)
d_i = torch.frombuffer(bytearray(inputs), dtype=torch.uint8).to(dev)
d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
stream = torch.cuda.current_stream(dev)
pkg.lib().bn254_set_profiling(1)
pkg.set_profile_kernels(None)
pvk.verify_batch_device(d_p.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), n, 256, 2, 0, stream.cuda_stream)
stream.synchronize()
prof, per = pvk.kernel_profile_all(0)
print(json.dumps({"status": list(d_s.cpu().numpy().tobytes()), "expected": list(exp), "launches": {k: v[0] for k, v in prof.items()}, "per_launch": per}))
"""


def test_lane_kernels_65_proofs(pkg, O):
    n = 65
    r = subprocess.run([sys.executable, "-c", _LANE_CHILD, ROOT, str(G16_SEED), str(n)], env=dict(os.environ, BN254_COOP="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    vk, proofs, inputs, exp = pkg.synth_groth16(G16_SEED, 2, n, invalid_every=8, agree=True, threads=8)
    assert bytes(out["expected"]) == exp
    assert set(exp) == {O.REJECT, O.ACCEPT, O.ERR_NOT_MEMBER, O.ERR_NOT_ON_CURVE, O.ERR_NOT_IN_SUBGROUP} and exp[64] == O.ACCEPT
    assert bytes(out["status"]) == exp
    assert bytes(out["status"]) == O.groth16_verify_many(proofs, 256, vk, inputs, 2, n, O.MODE_REFERENCE)
    # the lane form ran, with the launches of the chain: per sub-batch 36 runs of squarings and 54 products, the last of them the one with the verdict
    la = out["launches"]
    assert not [k for k in la if "coop" in k], la
    subs = la["k_f12_cyclo_sqr_n"] // FINAL_EXP_RUNS
    assert subs >= 1 and la["k_f12_cyclo_sqr_n"] == FINAL_EXP_RUNS * subs, la
    # (the verdict product is profiled as k_f12_mul; a batch this small runs its three Miller chains side by side: two copies of f = 1 and two products join them)
    joins = la.get("k_f12_copy", 0)
    assert joins in (0, 2 * subs) and la["k_f12_mul"] == FINAL_EXP_PRODUCTS * subs + joins, la
    assert la["k_f12_cyclo_sqr"] == 6 * subs, la


def test_cooperative_kernel_6_proofs(pkg, O, torch_dev):
    """one valid proof and one of each failure class: proofs 0, 7, 15, 23, 31, 39 of a stream with every 8th proof invalid (a proof depends on the seed and its index alone)"""
    vk, proofs, inputs, exp = pkg.synth_groth16(G16_SEED, 2, 40, invalid_every=8, agree=True, threads=8)
    pick = [0, 7, 15, 23, 31, 39]
    p6 = b"".join(proofs[256 * i:256 * i + 256] for i in pick); i6 = b"".join(inputs[64 * i:64 * i + 64] for i in pick); e6 = bytes(exp[i] for i in pick)
    assert e6[0] == O.ACCEPT and sorted(e6[1:]) == sorted([O.REJECT, O.REJECT, O.ERR_NOT_MEMBER, O.ERR_NOT_ON_CURVE, O.ERR_NOT_IN_SUBGROUP])
    pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
    try:
        got = _g16_device(torch_dev, pvk, p6, i6, 6)
        assert got == e6
        assert got == O.groth16_verify_many(p6, 256, vk, i6, 2, 6, O.MODE_REFERENCE)
        assert pvk.verify_batch(p6, i6, n=6) == e6
    finally:
        pvk.close()


def test_plonk_5_proofs(pkg, O, torch_dev):
    """The generator has six failure classes, so two batches of five: a valid proof with classes 0 - 3, then classes 4 and 5 between two valid proofs and class 0 again."""
    torch, dev = torch_dev
    n_public, n_qcp, log2 = PLONK_SHAPE
    vk, proofs, inputs, exp = pkg.synth_plonk(PLONK_SEED, n_public, n_qcp, log2, 48, invalid_every=8, threads=8)
    plen, ilen = 808 + 96 * n_qcp, 32 * n_public
    assert {exp[8 * k + 7] for k in range(6)} == {3, 2, 8, 7, 9} and exp[0] == exp[1] == exp[2] == pkg.ACCEPT
    pvk = pkg.PreparedPlonkVk(vk)
    try:
        for pick in ([0, 7, 15, 23, 31], [39, 1, 47, 2, 7]):
            pb = b"".join(proofs[plen * i:plen * (i + 1)] for i in pick); ib = b"".join(inputs[ilen * i:ilen * (i + 1)] for i in pick); want = bytes(exp[i] for i in pick)
            d_p = torch.frombuffer(bytearray(pb), dtype=torch.uint8).to(dev); d_i = torch.frombuffer(bytearray(ib), dtype=torch.uint8).to(dev)
            d_s = torch.full((5,), 0xEE, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev)
            pvk.verify_batch_device(d_p.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), 5, proof_stride=plen, n_public=n_public, device=dev.index, stream=stream.cuda_stream)
            stream.synchronize()
            got = bytes(d_s.cpu().numpy().tobytes())
            assert got == want, (pick, list(got), list(want))
            ref = bytes(O.plonk_verify(pb[plen * j:plen * (j + 1)], vk, [ib[ilen * j + 32 * s:ilen * j + 32 * s + 32] for s in range(n_public)]) for j in range(5))
            assert got == ref, (pick, list(got), list(ref))
    finally:
        pvk.close()
