"""One scenario of tests/test_gpu_selftest.py in a process of its own (the automatic self-test runs once per process and device, and BN254_SELFTEST is read when
the library is loaded): `python tests/selftest_child.py <scenario>` prints one JSON line.  Not a test module."""
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: one HIP runtime per process, tests/conftest.py)

pkg = importlib.import_module("snark-bn254-verifier_amd")
SEED, N = 0x5E1F0001, 16


def g16_batch():
    return pkg.synth_groth16(SEED, 2, N, invalid_every=4, agree=True, threads=2)


def plonk_batch():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "fixtures.json")))
    vk = open(os.path.join(ROOT, "tests", "golden", "plonk_vk.bin"), "rb").read()
    pl = [(bytes.fromhex(f["raw_proof"]), [int(x) for x in f["public_inputs"]]) for f in fx.values() if f["variant"] == "plonk"]
    pl.append((pl[0][0], [pl[0][1][0], pl[0][1][1] ^ 1]))
    return vk, b"".join(p.ljust(904, b"\0") for p, _ in pl), b"".join(int(x).to_bytes(32, "big") for _, xs in pl for x in xs), len(pl)


def raw_g16(pvk, proofs, inputs, n):
    st = (C.c_uint8 * (n + 8))(*([0xEE] * (n + 8)))
    rc = pkg.lib().bn254_groth16_verify_batch(pvk._h, proofs, 256, inputs, 2, n, st, 0, 0)
    return rc, bytes(st)


def raw_plonk(ppvk, proofs, inputs, n):
    st = (C.c_uint8 * (n + 8))(*([0xEE] * (n + 8)))
    rc = pkg.lib().bn254_plonk_verify_batch(ppvk._h, proofs, 904, inputs, 2, n, st, 0)
    return rc, bytes(st)


def main(scenario):
    out = {"state_at_load": pkg.selftest_state(0)[0]}
    if scenario in ("groth16", "skipped"):
        vk, proofs, inputs, _ = g16_batch()
        pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
        out["state_after_prepare"] = pkg.selftest_state(0)[0]
        out["status"] = list(pvk.verify_batch(proofs[:256], inputs[:64]))
        out["state_after_first_call"] = pkg.selftest_state(0)[0]
        if scenario == "skipped":
            rep = pkg.device_selftest(0)
            out["explicit"] = [rep["passed"], rep["mask"]]
            out["state_after_explicit"] = pkg.selftest_state(0)[0]
    elif scenario == "plonk":
        vk, proofs, inputs, n = plonk_batch()
        ppvk = pkg.PreparedPlonkVk(vk)
        out["status"] = list(ppvk.verify_batch(proofs, inputs))
        out["state_after_first_call"] = pkg.selftest_state(0)[0]
    elif scenario == "reserve":
        vk, proofs, inputs, _ = g16_batch()
        pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
        pvk.reserve(64)
        out["state_after_first_call"] = pkg.selftest_state(0)[0]
    elif scenario == "refusal":
        vk, proofs, inputs, _ = g16_batch()
        pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
        pvkb, pp, pi, pn = plonk_batch()
        ppvk = pkg.PreparedPlonkVk(pvkb)
        rc, mask, text = pkg.dbg_selftest(0, 4, record=True)
        out["inject"] = [rc, mask, text]
        out["state_after_inject"] = list(pkg.selftest_state(0))
        rc, st = raw_g16(pvk, proofs, inputs, N)
        out["g16_refused"] = [rc, pkg.lib().bn254_last_error().decode(), st == b"\xee" * (N + 8)]
        rc, st = raw_plonk(ppvk, pp, pi, pn)
        out["plonk_refused"] = [rc, pkg.lib().bn254_last_error().decode(), st == b"\xee" * (pn + 8)]
        try:
            pvk.verify_batch(proofs, inputs)
            out["raised"] = None
        except pkg.Bn254Error as e:
            out["raised"] = [type(e).__name__, e.code]
        rep = pkg.device_selftest(0)
        out["explicit"] = [rep["passed"], rep["mask"], rep["failed"]]
        out["state_after_explicit"] = list(pkg.selftest_state(0))
        rc, st = raw_g16(pvk, proofs, inputs, N)
        out["g16_after"] = [rc, list(st[:N]), st[N:] == b"\xee" * 8]
        rc, st = raw_plonk(ppvk, pp, pi, pn)
        out["plonk_after"] = [rc, list(st[:pn])]
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
