"""The cooperative form of the pairing check of a PlonK batch over a key list (k_coop12_miller_fixed_keys, csrc/bn254_coop12.hip: twelve lanes per slot, the line
tables of the slot's key fetched per lane; bn254_set_plonk_keys_params) on the GPU: the kernel's GT values against the oracle with keys that alternate inside a
wavefront, and the status bytes of small lists in that form against the generator, one single-key call per key and the oracle, with the lane form giving the same
bytes.  One process, every case finite; no case is meant to fault."""
import random

import pytest

from plonk_keys_common import A, B, C, D, Batch, check, diff, get_key, shuffled

pytestmark = pytest.mark.gpu

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


@pytest.fixture
def coop_knob(pkg):
    """the knob at its value of before the test, whatever the test does to it"""
    before = pkg.dbg_plonk_keys_knobs()[0]
    try:
        yield before
    finally:
        pkg.set_plonk_keys_params(before)


def _kzg_g2(O, key):
    """the two KZG G2 points of a PlonK key from its vk bytes (bn254_plonk.hpp::parse_plonk_vk: behind the 372 header bytes and the n_qcp commitment points come the
    KZG G1 generator, 32 bytes, and the two G2 points, 64 bytes each, compressed in the reference's flag convention)"""
    off = 372 + 32 * key.shape[1] + 32
    out = []
    for t in range(2):
        st, q = O.decompress_g2(key.vk[off + 64 * t:off + 64 * t + 64], O.MODE_REFERENCE)
        assert st == O.ACCEPT
        out.append(q)
    return out


def _gt_product(O, pairs):
    """prod e(P, Q) over the pairs whose G1 point is not the identity"""
    pairs = [(p, q) for p, q in pairs if p is not None]
    if not pairs:
        return (1).to_bytes(32, "big") + bytes(352)
    return O.pairing(b"".join(p for p, _ in pairs), b"".join(q for _, q in pairs))


def test_kernel_values_with_the_key_per_item(pkg, O, torch_dev):
    """k_coop12_miller_fixed_keys in its store mode on the tables of three prepared keys: the GT value of item i is e(P0_i, Q0_k) e(P1_i, Q1_k), final exponentiation
    included, with k = key_words[i >> key_shift] and Q0_k = kzg_g2[0], Q1_k = kzg_g2[1] of that key AS PARSED, with no negation: bn254_plonk_vk_prepare builds
    table 0 from the lines of kzg_g2[0] and table 1 from those of kzg_g2[1] (the check is e(P0, g2[0]) e(P1, g2[1]) == 1, and the sign of the second pairing is in
    P1 and in the key's own g2[1]); unlike a Groth16 key in gnark mode, whose tables hold the lines of -gamma and -delta.  13 items with the keys alternating
    inside every wavefront (three wavefronts, the last with three items and two idle groups) and one key word per item; then 130 items with one word per 64, where
    items 63 and 64 -- different keys -- sit in wavefront 12.  The identity flag on each pair in turn makes that pair's factor 1 whatever bytes the point holds.  An
    item that read a neighbour's tables cannot pass: for the same two points the expected values of any two keys differ, which is asserted."""
    keys = [get_key(pkg, s) for s in (A, B, C)]
    ks = pkg.PlonkKeySet([k.pvk for k in keys])
    g2 = [_kzg_g2(O, k) for k in keys]
    rng = random.Random(0xC0FE)
    pt = lambda: O.g1_mul(O.g1_gen(), rng.randrange(1, R))

    def expect(k, p0, p1, fl):
        return _gt_product(O, [(None if fl & 1 else p0, g2[k][0]), (None if fl & 2 else p1, g2[k][1])])

    p0, p1 = [pt() for _ in range(130)], [pt() for _ in range(130)]
    same = [expect(k, p0[0], p1[0], 0) for k in range(3)]
    assert len(set(same)) == 3, "two keys give the same value for the same points: the test could not tell their tables apart"
    assert len({expect(k, p0[0], p1[0], 2) for k in range(3)}) == 3 and len({expect(k, p0[0], p1[0], 1) for k in range(3)}) == 3      # each table alone tells them apart
    n = 13
    words = [(i + i // 5) % 3 for i in range(n)]       # 0 1 2 0 1 | 0 1 2 0 1 | 0 1 2: every wavefront holds all three keys
    assert all(len(set(words[w:w + 5])) == 3 for w in (0, 5)) and len(set(words[10:])) == 3
    for flags in ([0] * n, [i % 3 for i in range(n)], [(i + 1) % 4 for i in range(n)], [3] * n):
        out = ks.dbg_coop12_miller_fixed(words, 0, b"".join(p0[:n]), b"".join(p1[:n]), bytes(flags))
        for i in range(n):
            assert out[i] == expect(words[i], p0[i], p1[i], flags[i]), (flags[i], i, words[i])
    n = 130
    words = [1, 2, 0]
    flags = [0 if 60 <= i < 65 else (i % 4) for i in range(n)]
    out = ks.dbg_coop12_miller_fixed(words, 6, b"".join(p0), b"".join(p1), bytes(flags))
    for i in range(n):
        assert out[i] == expect(words[i >> 6], p0[i], p1[i], flags[i]), (i, words[i >> 6], flags[i])
    # a key word outside the list reads key 0, nothing else
    out = ks.dbg_coop12_miller_fixed([7, 1], 0, b"".join(p0[:2]), b"".join(p1[:2]), bytes(2))
    assert out[0] == expect(0, p0[0], p1[0], 0) and out[1] == expect(1, p0[1], p1[1], 0)


def _cases(pkg):
    a, b, c, d = (get_key(pkg, s) for s in (A, B, C, D))
    two = [a, c]
    cases = [("n = 1", Batch(two, [(1, 5)]))]
    for ca, cc in ((63, 1), (64, 1), (65, 64)):
        cases.append(("runs of %d and %d" % (ca, cc), Batch(two, shuffled([ca, cc], seed=ca))))
    cases.append(("an entry without proofs", Batch([a, d, c], [(0, j) for j in range(70)] + [(2, j) for j in range(9)])))
    cases.append(("a handle listed twice", Batch([a, c, a], [(0 if j % 2 else 2, j) for j in range(100)] + [(1, j) for j in range(30)])))
    return cases


def _parity(pkg, O, torch_dev, what, b, want_passes=None):
    ks = b.key_set(pkg)
    ks.reserve(b.n, proof_stride=b.proof_stride)
    plan = pkg.dbg_plonk_keys_plan(b.n, len(b.key_list), b.slots())
    passes = len(plan["pass_first"])
    if want_passes is not None:
        assert passes == want_passes and plan["workers"] == want_passes
    assert plan["per_pass"] <= pkg.dbg_plonk_keys_knobs()[0]
    s0 = ks.state()
    got = b.host(ks)
    s1 = ks.state()
    check(pkg, O, b, got, what + ", host buffers")
    dev = b.device(ks, torch_dev)
    s2 = ks.state()
    assert dev == got, what + ", device entry: " + diff(dev, got)
    assert s1[3] - s0[3] == passes and s2[3] - s1[3] == passes, (what, s0, s1, s2, passes)
    assert s2[:3] == s0[:3]                                  # no flag, no joint check
    pkg.set_plonk_keys_params(0)                             # the lane form: the same bytes
    lane_h, lane_d = b.host(ks), b.device(ks, torch_dev)
    assert lane_h == got and lane_d == got, what + ", lane form: " + (diff(lane_h, got) or diff(lane_d, got))
    assert ks.state()[3] == s2[3]


def test_parity_of_small_lists_in_the_cooperative_form(pkg, O, torch_dev, coop_knob):
    """the edges of the granule, an entry without proofs, a handle listed twice: every pass in the cooperative form (counted), then in the lane form (not counted)"""
    assert coop_knob >= 6450, "the default of the knob must cover the batches of this file"
    for what, b in _cases(pkg):
        pkg.set_plonk_keys_params(coop_knob)
        _parity(pkg, O, torch_dev, what, b)


def test_parity_of_two_chains_in_the_cooperative_form(pkg, O, torch_dev, coop_knob):
    """6450 proofs of three keys: two chains with the cut inside a key's run (2112 + 2176 > 3264 > 2112), two cooperative passes side by side"""
    kl = [get_key(pkg, s) for s in (A, C, D)]
    b = Batch(kl, shuffled([2100, 2150, 2200]), proof_stride=1000, input_stride=160)
    _parity(pkg, O, torch_dev, "6450 proofs of three keys", b, want_passes=2)
