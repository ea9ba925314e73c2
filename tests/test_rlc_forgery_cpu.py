"""The cancelling forgeries of tests/rlc_forgery.py without a GPU:

- the groups of a BN254_FLAG_RLC chunk as the enqueue computes them (bn254_dbg_g16_rlc_groups: the function g16_enqueue_rlc plans by) against a Python
  mirror of the fold rule of csrc/bn254_rlc_plan.h -- the membership the GPU tests plant their pairs by;
- the vectors themselves, judged by the oracle's pairings: each forged proof fails alone, the pair passes under equal weights (and under weights 1, k for C_a + k T);
- the shared fold and group code (tests/hostsim: hs_rlc_pipeline) lets the pair through when every proof draws the same ChaCha20 block (the stand-in's
  weight_mode 1) and refuses it under the real draw -- the property tests/test_gpu_rlc_forgery.py relies on."""
import ctypes as C
import hashlib
import os
import random

import pytest

from rlc_forgery import GT_ONE, R, fold_bits, fold_group_of, fold_halves, forge_c, forge_x, g1_neg, members_by_group, plonk_pair, x_positions
from test_rlc_hostsim import _key_points
from test_rlc_wide_cpu import _parts, _share


def _env_int(name, default, lo, hi):
    return min(hi, max(lo, int(os.environ.get(name, default))))


@pytest.fixture()
def share_knob(pkg):
    """share_min_lanes for one test; afterwards what the library read when it was loaded."""
    yield lambda v: pkg.set_rlc_params(share_min_lanes=v)
    pkg.set_rlc_params(share_min_lanes=int(os.environ.get("BN254_RLC_SHARE_MIN_LANES", "65536")))


@pytest.mark.parametrize("min_lanes", [1, 65536])
@pytest.mark.parametrize("m", [64, 67, 257, 1000, 4133, 16347, 16384, 40000])
def test_groups_as_the_enqueue_plans_them(pkg, share_knob, m, min_lanes):
    share_knob(min_lanes)
    lg, ls = _env_int("BN254_RLC_GROUP_LOG2", 5, 1, 16), _env_int("BN254_RLC_SHARE_LOG2", 3, 0, 3)
    group, share = pkg.dbg_rlc_groups(m)
    want_group, want_share, base = [], [], 0
    for lo, hi in _parts(m, _env_int("BN254_STREAMS", 2, 1, 4)):
        s = _share(hi - lo, lg, ls, min_lanes)
        half, groups = fold_halves(hi - lo, lg, s)
        want_group += [base + fold_group_of(i, half) for i in range(hi - lo)]
        want_share += [s] * (hi - lo)
        for g, mem in members_by_group(want_group[lo:hi]).items():
            assert len(mem) <= 1 << len(half)                                     # no group beyond 2^rounds members ...
            assert len({fold_bits(i, half) for i in mem}) == len(mem)            # ... each with fold bits of its own
        base += groups
    assert group == want_group and share == want_share
    assert sorted(set(group)) == list(range(base))                                # every group id is hit
    if m == 40000 and "BN254_STREAMS" not in os.environ:
        assert group[20224] == 632 and share[0] == (3 if min_lanes == 1 else 0)   # two launch parts, of 20224 (632 groups) and 19776 proofs
    if m == 16384 and min_lanes == 65536 and lg == 5:
        assert base == 512 and group[:512] == list(range(512)) and group[512] == 0


# ---- the vectors, by the oracle ----------------------------------------------------------------------------------------------------------------------------------
def _prod(O, terms):
    """prod e(P, Q) over (P, Q) pairs, as GT bytes."""
    return O.pairing(b"".join(p for p, _ in terms), b"".join(q for _, q in terms))


def _g16_terms(O, kp, proof, xs, scale=1):
    """The four pairs of e(A,B) e(L,-gamma) e(C,-delta) e(-alpha,beta) of one proof, its G1 arguments scaled."""
    alpha, ks, qg, qd, qb = kp
    L = ks[:64]
    for j, x in enumerate(xs):
        L = O.g1_add(L, O.g1_mul(ks[64 * (j + 1):64 * (j + 2)], x % R))
    g1 = [proof[:64], L, proof[192:256], g1_neg(alpha)]
    return list(zip([O.g1_mul(p, scale % R) for p in g1], [proof[64:192], qg, qd, qb]))


def _rows(inputs, n_public, i):
    return [int.from_bytes(inputs[32 * (n_public * i + j):32 * (n_public * i + j + 1)], "big") for j in range(n_public)]


@pytest.mark.parametrize("n_public", [2, 9])
def test_groth16_pairs_cancel_under_equal_weights(pkg, O, n_public):
    vk, proofs, inputs, exp = pkg.synth_groth16(0xB2548000 + n_public, n_public, 2, invalid_every=0, agree=True, threads=2)
    kp = _key_points(pkg, vk, n_public)
    rng = random.Random(n_public)

    def check(p, x, k=1):
        p, x = bytes(p), bytes(x)
        assert O.groth16_verify_many(p, 256, vk, x, n_public, 2, O.MODE_GNARK) == bytes([O.REJECT] * 2)
        each = [_g16_terms(O, kp, p[256 * i:256 * (i + 1)], _rows(x, n_public, i)) for i in (0, 1)]
        assert _prod(O, each[0]) != GT_ONE and _prod(O, each[1]) != GT_ONE         # each fails alone
        # weights (1, k): r_b = k r_a.  The proof that carries -T is the one scaled by k.
        assert _prod(O, each[0] + _g16_terms(O, kp, p[256:], _rows(x, n_public, 1), k)) == GT_ONE
        if k != 1:
            assert _prod(O, each[0] + each[1]) != GT_ONE

    assert _prod(O, _g16_terms(O, kp, proofs[:256], _rows(inputs, n_public, 0))) == GT_ONE       # the valid proof, as a check of this arithmetic
    for k in (1, -1, 2):
        p = bytearray(proofs)
        forge_c(O, p, 0, 1, O.g1_mul(O.g1_gen(), rng.randrange(1, R)), k)
        check(p, inputs, k)
    for j in x_positions(n_public):
        x = bytearray(inputs)
        forge_x(x, n_public, 0, 1, j, rng.randrange(1, R))
        check(proofs, x)


def test_plonk_pair_cancels_under_any_two_lambdas(O, fixtures):
    fx, vk = fixtures
    f = fx["fibonacci_plonk"]
    proof, pis = bytes.fromhex(f["raw_proof"]), [int(x) for x in f["public_inputs"]]
    rng = random.Random(3)
    copies = plonk_pair(O, proof, O.g1_mul(O.g1_gen(), rng.randrange(1, R)))
    lams = (rng.getrandbits(128) | 1, rng.getrandbits(128) | 2)
    assert lams[0] != lams[1]
    sums = [bytes(64), bytes(64)]
    for c, lam in zip(copies, lams):
        st, ps, qs = O.plonk_pairing_inputs_lam(c, vk, pis, lam)
        assert st == O.ERR_PAIRING_FAILED and O.plonk_verify(c, vk, pis) == O.ERR_PAIRING_FAILED
        assert _prod(O, list(zip(ps, qs))) != GT_ONE
        sums = [O.g1_add(s, p) for s, p in zip(sums, ps)]
    assert _prod(O, list(zip(sums, qs))) == GT_ONE
    st, ps, _ = O.plonk_pairing_inputs_lam(proof, vk, pis, lams[0])
    assert st == O.ACCEPT and _prod(O, list(zip(ps, qs))) == GT_ONE


# ---- equal weights accept the pair, the real draw rejects it: the shared fold and group code on the host -----------------------------------------------------------
@pytest.mark.parametrize("log2_share", [0, 1])
def test_hostsim_equal_weights_let_the_pair_through(hostsim, pkg, O, log2_share):
    n, n_public = 4, 2
    vk, proofs, inputs, exp = pkg.synth_groth16(0xB2548100, n_public, n, invalid_every=0, agree=True, threads=2)
    kp = _key_points(pkg, vk, n_public)
    key = hashlib.sha256(b"rlc-forgery-key").digest() + bytes(12)
    rng = random.Random(11)

    def run(p, x, weight_mode):
        groups = (C.c_uint8 * n)(); group_of = (C.c_uint32 * n)()
        ng = hostsim.hs_rlc_pipeline(n, bytes(p), bytes(x), n_public, kp[0], kp[1], kp[2], kp[3], kp[4], key, 8, 0, groups, group_of, log2_share, weight_mode)
        assert ng == 1 and list(group_of) == [0] * n
        return groups[0]

    assert run(proofs, inputs, 0) == 1 and run(proofs, inputs, 1) == 1
    a, b = 0, 3                        # log2_share 1: two lanes; proofs 0 and 3 sit in different lanes and at different places of them
    pc = bytearray(proofs); forge_c(O, pc, a, b, O.g1_mul(O.g1_gen(), rng.randrange(1, R)))
    px = bytearray(inputs); forge_x(px, n_public, a, b, 0, rng.randrange(1, R))
    for p, x in ((pc, inputs), (proofs, px)):
        st = O.groth16_verify_many(bytes(p), 256, vk, bytes(x), n_public, n, O.MODE_GNARK)
        assert list(st) == [0 if i in (a, b) else 1 for i in range(n)]
        assert run(p, x, 1) == 1       # every proof draws counter 0: the errors cancel and the forged group passes
        assert run(p, x, 0) == 0       # independent weights: it fails
