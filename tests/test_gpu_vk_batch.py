"""bn254_groth16_vk_prepare_batch on the GPU (include/bn254_verify.h, "Many keys prepared in one call"): k_vkp_dec_g1 / k_vkp_dec_g2 / k_vkp_fold / k_vkp_lines
and the one-pair pairing program over the keys of a pass.

The definition of correctness is the header's and the same as in tests/test_vk_batch_cpu.py: per key the status is bn254_groth16_vk_prepare's return code, the handle
is NULL or has the single-key handle's host image dword for dword, and every entry point gives the same status bytes with it.  The single-key image of every distinct
(key, mode) is computed once on the host and shared by the cases (3 - 6 ms each: that bounds the sizes); the lists repeat the keys of a small pool, which moves them
over the lanes without preparing more references.  One process but for the pass-size knob, which a library reads once; no case is meant to fault."""
import os
import subprocess
import sys

import pytest

from test_gpu_multikey import Key, Mixed
from test_vk_batch_cpu import E_VK, OK, _single, _synth_vk, _without_k, bad_keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (0, 1, 5, 16, 17, 40)


class Pool:
    """distinct keys and, per (key, mode), the single-key entry's answer: (return code, image or None), computed when first asked for"""

    def __init__(self, pkg):
        self.pkg = pkg
        self.two = [_synth_vk(pkg, 0x5C0000 + i, 2, agree=bool(i % 3)) for i in range(24)]     # 2-input keys; every third with root orders that differ between the modes
        self.mixed = [_synth_vk(pkg, 0x5C1000 + w, w) for w in WIDTHS] + [_without_k(_synth_vk(pkg, 0x5C1000, 0))]
        self.wide = _synth_vk(pkg, 0x5C2000, 300)                                              # 304 G1 lanes: the decode kernel crosses blocks within one key
        self.ref = {}

    def single(self, vk, mode):
        if (vk, mode) not in self.ref:
            rc, k = _single(self.pkg, vk, mode)
            self.ref[(vk, mode)] = (rc, self.pkg.dbg_pvk_image(k) if k else None)
            if k:
                k.close()
        return self.ref[(vk, mode)]

    def list_of(self, n):
        """n keys: 2-input keys with the other widths mixed in at every 7th place and the 300-input key in the middle"""
        out = [self.mixed[(i // 7) % len(self.mixed)] if i % 7 == 3 else self.two[i % len(self.two)] for i in range(n)]
        out[n // 2] = self.wide
        return out

    def check(self, vks, mode, keys, status):
        assert len(keys) == len(status) == len(vks)
        for i, vk in enumerate(vks):
            rc, image = self.single(vk, mode)
            assert status[i] == rc, (i, status[i], rc)
            assert (keys[i] is None) == (image is None), i
            if image is not None:
                assert self.pkg.dbg_pvk_image(keys[i]) == image, "image of key %d of %d differs (mode %d)" % (i, len(vks), mode)


@pytest.fixture(scope="module")
def pool(pkg):
    return Pool(pkg)


def _close(keys):
    for k in keys:
        if k is not None:
            k.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_images_equal_the_single_key_images(pkg, pool, mode):
    """list sizes around the wavefront and block boundaries of the per-key kernels (64 lanes a block), the per-point kernels far beyond theirs"""
    for n in (1, 63, 64, 65, 300):
        vks = pool.list_of(n)
        keys, status = pkg.prepare_vks(vks, mode, 0, with_status=True)
        assert status == [OK] * n
        pool.check(vks, mode, keys, status)
        _close(keys)


@pytest.mark.parametrize("mode", [0, 1])
def test_bad_keys_at_lane_boundaries(pkg, pool, mode):
    """keys that do not load at positions 0, 31, 63 and 64 of a 130-key list -- two that get no lanes (the host's scan refuses them) and two whose points fail on the
    device: statuses and NULLs as the single-key entry has them, every good key image-equal"""
    bad = dict(bad_keys(pkg, pool.two[0], 2, mode))
    vks = pool.list_of(130)
    vks[0] = bad["G2 x without a root (gamma)"]
    vks[31] = bad["truncated at 288"]
    vks[63] = bad["flag 00 at %d" % (292 + 32 * 2)]
    vks[64] = bad["K count larger than the buffer"]
    keys, status = pkg.prepare_vks(vks, mode, 0, with_status=True)
    assert [i for i, s in enumerate(status) if s != OK] == [0, 31, 63, 64] and {status[i] for i in (0, 31, 63, 64)} == {E_VK}
    pool.check(vks, mode, keys, status)
    _close(keys)
    # the probe with a device ordinal runs the same kernels and reports their times
    keys, status, ms = pkg.dbg_prepare_vks(vks[:66], mode, 0)
    pool.check(vks[:66], mode, keys, status)
    assert set(ms) == set(pkg.VK_PREPARE_STAGES) and all(v > 0 for v in ms.values()), ms
    _close(keys)


_PASS_SCRIPT = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import importlib
pkg = importlib.import_module("snark-bn254-verifier_amd")
from test_gpu_vk_batch import Pool
pool = Pool(pkg)
vks = pool.list_of(300)
vks[130] = vks[130][:200]
for mode in (0, 1):
    keys, status = pkg.prepare_vks(vks, mode, 0, with_status=True)
    assert [i for i, s in enumerate(status) if s] == [130]
    pool.check(vks, mode, keys, status)
print("passes ok")
"""


def test_a_list_longer_than_one_pass():
    """BN254_VKPREP_PASS=128 (read once, when the library is loaded: hence a process of its own): 300 keys are three passes, with a key that gets no lanes in the second"""
    env = dict(os.environ, BN254_VKPREP_PASS="128")
    r = subprocess.run([sys.executable, "-c", _PASS_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "passes ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("n", [256, 40000])     # cooperative kernels / lane kernels
def test_verdicts_through_the_single_key_entry(pkg, n):
    vk, proofs, inputs, exp = pkg.synth_groth16(0x5C3000 + n, 2, n, invalid_every=5, agree=True, threads=16)
    assert len(set(exp)) >= 4
    for mode in (pkg.VK_REFERENCE, pkg.VK_GNARK):
        batch, = pkg.prepare_vks([vk], mode, 0)
        host = pkg.PreparedVk(vk, mode)
        got = batch.verify_batch(proofs, inputs, n)
        assert got == exp and got == host.verify_batch(proofs, inputs, n)
        batch.close(); host.close()


def test_verdicts_through_a_key_list_and_mixed_handles(pkg):
    """65 keys, 2000 proofs, the grouped and the direct form: handles of the batch entry, and a list that mixes them with host-prepared ones; then the handles are freed
    in an order of their own"""
    widths = (0, 1, 2, 5, 16)
    ks = [Key(pkg, 0x5C4000 + i, widths[i % 5], 30 + (i % 3), mode=i % 2, invalid_every=5, threads=8) for i in range(65)]
    mx = Mixed(ks, seed=5)
    assert 1900 <= len(mx.entries) <= 2100
    by_mode = {m: pkg.prepare_vks([k.vk for k in ks if k.mode == m], m, 0) for m in (0, 1)}
    fresh = [by_mode[k.mode].pop(0) for k in ks]
    lo, hi = 0, 30721                                   # the hand-over the library starts with (the knob has no getter)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pkg.dbg_keys_plan(mid, 1)[0] == 1 else (lo, mid)
    try:
        for coop_max, form in ((0, 0), (30720, 1)):
            pkg.set_keys_params(coop_max)
            want = mx.run(mx.key_set(pkg))              # host-prepared handles
            assert want == mx.exp
            for handles in (fresh, [f if i % 2 else k.pvk for i, (f, k) in enumerate(zip(fresh, ks))]):
                kset = pkg.KeySet(handles)
                assert mx.run(kset) == want
                assert kset.last_form() == form
    finally:
        pkg.set_keys_params(lo)
    for i in sorted(range(65), key=lambda i: (i * 37) % 65):
        (fresh[i] if i % 3 else ks[i].pvk).close()
    for i in range(65):
        (ks[i].pvk if i % 3 else fresh[i]).close()
