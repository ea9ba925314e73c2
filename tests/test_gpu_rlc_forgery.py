"""Cancelling forgeries against BN254_FLAG_RLC on the GPU (tests/rlc_forgery.py; the vectors and the property are checked without a GPU in
tests/test_rlc_forgery_cpu.py): pairs of invalid proofs whose errors cancel whenever their two batching weights coincide, planted one pair per group, at every
pair of places inside a group the kernels could give the same weight -- two lanes, two proofs of a shared-accumulator lane, the partners of every fold round.
A forged proof that comes back ACCEPT is an accepted forgery.

Groth16: k_rlc_scale / k_rlc_scale_wide (the weight draw), the RLC_W parking and rlc_group_scalar / k_rlc_group_scalars (wide keys, the three table forms), 1 and
8 proofs per Miller-loop lane, compressed records.  Membership comes from bn254_dbg_g16_rlc_groups, the plan the enqueue itself makes.
PlonK: pl_stage2_body's weight of a proof (single key) or slot (key lists, cooperative and lane form), groups of 64."""
import itertools
import os
import random
import zlib

import pytest

from kzg_forgery import OFF_H
from plonk_keys_common import A, B, G, PAIRING_FAILED, Batch, diff, get_key
from rlc_forgery import R, fold_bit_pair, fold_group_of, fold_halves, forge_c, forge_x, members_by_group, plonk_pair, x_positions

pytestmark = pytest.mark.gpu
N_FULL, N_ODD = 16384, 16347
_WL = {}


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _rlc_always(pkg):
    """The RLC kernels on every call (tests/test_gpu_round2.py: from 64 proofs, no adaptive bypass -- which lowers the threshold of the wide keys with it, as
    tests/test_gpu_rlc_wide.py does); afterwards the defaults, and share_min_lanes as the library read it when it was loaded."""
    pkg.set_rlc_params(min_batch=64, adaptive=0, share_min_lanes=-1)
    yield
    pkg.set_rlc_params(min_batch=200000, adaptive=1, share_min_lanes=int(os.environ.get("BN254_RLC_SHARE_MIN_LANES", "65536")))


def _workload(pkg, n_public):
    """One valid workload of N_FULL proofs per key, generated once and never changed (the batches are copies)."""
    if n_public not in _WL:
        vk, proofs, inputs, exp = pkg.synth_groth16(0xB2549000 + n_public, n_public, N_FULL, invalid_every=0, agree=True, threads=16)
        assert exp == bytes([pkg.ACCEPT]) * N_FULL
        _WL[n_public] = (vk, proofs, inputs)
    return _WL[n_public]


def _plant_plan(pkg, n, seed):
    """[(a, b)], one pair per planted group, and the proofs of the planted groups.  Groups as the enqueue forms them now; slots: a group's members in order."""
    group, share = pkg.dbg_rlc_groups(n)
    by_group = members_by_group(group)
    gids = sorted(by_group)
    rng = random.Random(seed)
    pairs = []
    if n == N_FULL:
        # every unordered pair of slots, one per group: 496 of the 512 groups of 32, the other 16 stay valid
        size = min(len(m) for m in by_group.values())
        for g, (x, y) in zip(gids, itertools.combinations(range(size), 2)):
            pairs.append((g, by_group[g][x], by_group[g][y]))
        if size == 32 and len(gids) == 512:
            assert len(pairs) == 496
    else:
        # the partners of every fold round (three settings of the other fold bits), the first and the last member, then seeded pairs: 240 of the 256 groups
        assert len(set(share)) == 1 and group == [fold_group_of(i, fold_halves(n, _log2_group(), share[0])[0]) for i in range(n)]
        half, _ = fold_halves(n, _log2_group(), share[0])
        todo = [(k, s) for k in range(len(half)) for s in range(3)] + ["ends"]
        for g in gids[:max(len(todo), len(gids) - 16)]:
            mem = by_group[g]
            what = todo.pop(0) if todo else None
            pr = fold_bit_pair(mem, half, what[0], what[1], rng) if isinstance(what, tuple) else (mem[0], mem[-1]) if what == "ends" else None
            pairs.append((g,) + tuple(pr if pr else rng.sample(mem, 2)))
        if len(gids) == 256:
            assert len(pairs) == 240
    assert len({g for g, _, _ in pairs}) == len(pairs) < len(gids)                  # never two pairs in a group, and some groups stay valid
    assert all(group[a] == group[b] == g and a != b for g, a, b in pairs)
    return [(a, b) for _, a, b in pairs], sum(len(by_group[g]) for g, _, _ in pairs)


def _log2_group():
    return min(16, max(1, int(os.environ.get("BN254_RLC_GROUP_LOG2", "5"))))


def _forge(O, family, proofs, inputs, n_public, pairs, seed):
    rng = random.Random(seed)
    proofs, inputs = bytearray(proofs), bytearray(inputs)
    gen = O.g1_gen()
    for a, b in pairs:
        if family[0] == "C":
            forge_c(O, proofs, a, b, O.g1_mul(gen, rng.randrange(1, R)), family[1])
        else:
            forge_x(inputs, n_public, a, b, family[1], rng.randrange(1, R))
    return bytes(proofs), bytes(inputs)


def _run(pkg, O, n_public, n, family, share_min_lanes=-1, compressed=False):
    """One batch: every forged proof REJECT and every other ACCEPT, under the flag and on the exact path; the fresh key's fallback share = the proofs of the planted
    groups / n, which holds only if an RLC pass ran, every planted group failed inside it and no valid group did.  Returns (planted groups, share)."""
    vk, proofs, inputs = _workload(pkg, n_public)
    pkg.set_rlc_params(share_min_lanes=share_min_lanes)
    pairs, in_planted = _plant_plan(pkg, n, 1000 * n_public + n)
    p, x = _forge(O, family, proofs[:256 * n], inputs[:32 * n_public * n], n_public, pairs, zlib.crc32(repr(family).encode()))
    forged = {i for ab in pairs for i in ab}
    assert len(forged) == 2 * len(pairs)
    want = bytes(pkg.REJECT if i in forged else pkg.ACCEPT for i in range(n))
    a, b = pairs[len(pairs) // 2]
    sample = [a, b, (a + 1) % n]
    sp, sx = b"".join(p[256 * i:256 * (i + 1)] for i in sample), b"".join(x[32 * n_public * i:32 * n_public * (i + 1)] for i in sample)
    assert O.groth16_verify_many(sp, 256, vk, sx, n_public, 3) == bytes(want[i] for i in sample)
    if compressed:
        p = b"".join(O.compress_g1(p[256 * i:256 * i + 64]) + O.compress_g2(p[256 * i + 64:256 * i + 192]) + O.compress_g1(p[256 * i + 192:256 * i + 256]) for i in range(n))
    pvk = pkg.PreparedVk(vk)
    try:
        assert pvk.rlc_state()[0] == -1.0
        rlc = pvk.verify_batch(p, x, n, flags=pkg.FLAG_RLC, compressed=compressed)
        share = pvk.rlc_state()[0]
        exact = pvk.verify_batch(p, x, n, compressed=compressed)
    finally:
        pvk.close()
    accepted = [i for i in sorted(forged) if rlc[i] == pkg.ACCEPT]
    where = [(a, b) for a, b in pairs if a in accepted or b in accepted]
    print("n_public %d n %d family %r share_min_lanes %d compressed %d: %d planted groups, fallback share %.6f" % (n_public, n, family, share_min_lanes, compressed, len(pairs), share))
    assert not accepted, "%d forged proofs ACCEPTED under BN254_FLAG_RLC; the first pairs (a, b): %r" % (len(accepted), where[:8])
    assert rlc == want, diff(rlc, want)
    assert exact == want, diff(exact, want)
    assert abs(share - in_planted / n) <= 2.0 ** -23, (share, in_planted / n)
    if n == N_FULL and _log2_group() == 5:
        assert in_planted / n == 0.96875
    return len(pairs), share


NARROW = [("C", 1), ("X", 0), ("X", 1)]


@pytest.mark.parametrize("share_min_lanes", [65536, 1])
@pytest.mark.parametrize("n", [N_FULL, N_ODD])
@pytest.mark.parametrize("family", NARROW)
def test_groth16_narrow_key(pkg, O, torch_dev, family, n, share_min_lanes):
    """n_public 2 (the t_j slots per lane): one proof per Miller-loop lane, and eight (every pre-fold round pairs two proofs of one lane)."""
    _run(pkg, O, 2, n, family, share_min_lanes)


@pytest.mark.parametrize("k", [-1, 2])
def test_groth16_narrow_key_other_ratios(pkg, O, torch_dev, k):
    """C_a + k T, C_b - T: passes exactly when r_b = k r_a -- weights that differ by a sign or a shift instead of being equal."""
    _run(pkg, O, 2, N_FULL, ("C", k))


def test_groth16_compressed_records(pkg, O, torch_dev):
    """Family C applied before compression with the oracle's encoder: the decompression scratch is what the RLC pass reads."""
    _run(pkg, O, 2, N_FULL, ("C", 1), compressed=True)


WIDE = [(8, ("X", 0)), (8, ("X", 7))] + [(w, f) for w in (9, 17, 40) for f in [("X", j) for j in x_positions(w)] + [("C", 1)]]


@pytest.mark.parametrize("n_public,family", WIDE)
def test_groth16_wider_keys(pkg, O, torch_dev, n_public, family):
    """8 inputs: the last narrow key.  9: group scalars with the 13-bit window tables; 17 and 40: with the comb tables, the public-input sum in one chunk of 16
    inputs and a rest, and in three chunks (X_j on both sides of every chunk boundary)."""
    _run(pkg, O, n_public, N_FULL, family)


def test_groth16_byte_window_tables(pkg, O, torch_dev, monkeypatch):
    """The third table form of a wide key (BN254_WIDE_COMB=0 when the key is prepared: byte windows instead of the comb), 17 inputs."""
    monkeypatch.setenv("BN254_WIDE_COMB", "0")
    for family in (("X", 0), ("X", 15), ("X", 16), ("C", 1)):
        _run(pkg, O, 17, N_FULL, family)


# ---- PlonK -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _lane_pairs(seed):
    """The lane pairs of a group of 64, one group each: (j, j xor m) for every m at j = 0 and at one seeded j, the ends, the middle."""
    rng = random.Random(seed)
    pairs = []
    for m in (1, 2, 4, 8, 16, 32):
        j = rng.choice([v for v in range(64) if v not in (0, m)])
        pairs += [(0, m), (min(j, j ^ m), max(j, j ^ m))]
    return pairs + [(0, 63), (31, 32)]


N_PLONK = 1019                 # 16 groups of 64, the last one of 59
PARTIAL_PAIR = (5, 58)


@pytest.fixture
def plonk_rlc_from_64(pkg):
    before = pkg.dbg_plonk_keys_knobs()[1]
    try:
        pkg.set_plonk_rlc_params(64)
        yield
    finally:
        pkg.set_plonk_rlc_params(before)


def test_plonk_single_key(pkg, O, fixtures, torch_dev, plonk_rlc_from_64):
    """1019 copies of the four valid fixture proofs in one pass: groups of 64 consecutive proofs.  14 groups with a pair (H + D, H - D) of one proof, one pair in
    the partial group, one group left valid."""
    fx, vk = fixtures
    cases = [(bytes.fromhex(f["raw_proof"]), b"".join(int(x).to_bytes(32, "big") for x in f["public_inputs"])) for f in fx.values() if f["variant"] == "plonk"]
    assert len(cases) >= 4 and all(len(c[0]) == 904 and len(c[1]) == 64 for c in cases)
    rng = random.Random(5)
    recs = [cases[i % len(cases)] for i in range(N_PLONK)]
    want = bytearray([pkg.ACCEPT]) * N_PLONK
    lanes = _lane_pairs(6) + [PARTIAL_PAIR]
    assert len(lanes) == 15 and N_PLONK - 64 * 15 > PARTIAL_PAIR[1]
    for g, (x, y) in zip([g for g in range(16) if g != 7][:14] + [15], lanes):         # group 7 stays valid
        proof, row = cases[(g + x) % len(cases)]
        plus, minus = plonk_pair(O, proof, O.g1_mul(O.g1_gen(), rng.randrange(1, R)))
        recs[64 * g + x], recs[64 * g + y] = (plus, row), (minus, row)
        want[64 * g + x] = want[64 * g + y] = PAIRING_FAILED
        if g in (0, 15):
            pis = [int.from_bytes(row[:32], "big"), int.from_bytes(row[32:], "big")]
            assert O.plonk_verify(plus, vk, pis) == O.plonk_verify(minus, vk, pis) == PAIRING_FAILED
    want = bytes(want)
    assert want.count(bytes([PAIRING_FAILED])) == 30
    p, q = b"".join(r[0] for r in recs), b"".join(r[1] for r in recs)
    pvk = pkg.PreparedPlonkVk(vk)
    try:
        rlc = pvk.verify_batch(p, q, N_PLONK, flags=pkg.FLAG_RLC)
        exact = pvk.verify_batch(p, q, N_PLONK)
    finally:
        pvk.close()
    accepted = [i for i in range(N_PLONK) if want[i] == PAIRING_FAILED and rlc[i] == pkg.ACCEPT]
    assert not accepted, "forged PlonK proofs ACCEPTED under BN254_FLAG_RLC at (group, lane): %r" % [(i // 64, i % 64) for i in accepted]
    assert rlc == want, diff(rlc, want)
    assert exact == want, diff(exact, want)


@pytest.mark.parametrize("form", ["cooperative", "lanes"])
def test_plonk_key_list(pkg, O, torch_dev, plonk_rlc_from_64, form):
    """Two synthetic keys in a list of sixteen entries, alternating, one entry per granule of 64 slots (the one that ends the batch holds 59 proofs), each granule one
    group with its key.  The same lane pairs, planted in slot order (bn254_dbg_g16_keys_group); the list's counters: one joint pass over 16 groups, 15 of them failed.

    The device places a key's proofs wavefront by wavefront in whatever order the wavefronts arrive (csrc/bn254_k_keys.hip::k_keys_place), and inside a wavefront in lane
    order.  So the 64 consecutive batch positions of every wavefront carry ONE entry's proofs here, all of them: slot = first slot of the entry + lane on every run, which
    the test checks on the device's own grouping before it relies on it."""
    ka, kb = get_key(pkg, A), get_key(pkg, B)
    key_list = [ka, kb] * 8
    entry_of_wave = list(range(16))
    random.Random(21).shuffle(entry_of_wave)
    used, items = {0: 0, 1: 0}, []
    valid = [k.numbers(lambda s: s == pkg.ACCEPT) for k in (ka, kb)]
    for w, e in enumerate(entry_of_wave):
        c = 64 if w < 15 else N_PLONK - 64 * 15
        items += [(e, j) for j in valid[e & 1][used[e & 1]:used[e & 1] + c]]
        used[e & 1] += c
    b = Batch(key_list, items)
    assert b.n == N_PLONK and b.exp == bytes([pkg.ACCEPT]) * b.n and b.plen == b.proof_stride == 904 and b.input_stride == 64
    s2p, gk, n_slots = pkg.dbg_keys_group(b.index, 16, device=-1)
    assert n_slots == 16 * G and list(gk[:16]) == list(range(16))
    for w, e in enumerate(entry_of_wave):
        assert all(s2p[G * e + l] == (G * w + l if G * w + l < b.n else 0xffffffff) for l in range(G))
    d_s2p, d_gk, d_slots = pkg.dbg_keys_group(b.index, 16, device=0)
    assert d_slots == n_slots and list(d_s2p[:n_slots]) == list(s2p[:n_slots]) and list(d_gk[:16]) == list(gk[:16])
    partial = entry_of_wave[15]
    full = [g for g in range(16) if g != partial]
    lanes = _lane_pairs(7)
    rng = random.Random(8)
    proofs, rows, want = bytearray(b.proofs), bytearray(b.rows), bytearray(b.exp)
    for g, (x, y) in list(zip(full[:7] + full[8:], lanes)) + [(partial, PARTIAL_PAIR)]:       # the eighth full granule stays valid
        ia, ib = s2p[G * g + x], s2p[G * g + y]
        assert b.index[ia] == b.index[ib] == gk[g]
        plus, minus = plonk_pair(O, bytes(proofs[904 * ia:904 * (ia + 1)]), O.g1_mul(O.g1_gen(), rng.randrange(1, R)))
        proofs[904 * ia:904 * (ia + 1)], proofs[904 * ib:904 * (ib + 1)] = plus, minus
        rows[64 * ib:64 * (ib + 1)] = rows[64 * ia:64 * (ia + 1)]
        want[ia] = want[ib] = PAIRING_FAILED
        if g == partial:
            key = key_list[g]
            pis = [bytes(rows[64 * ia + 32 * t:64 * ia + 32 * t + 32]) for t in range(key.n_public)]
            assert O.plonk_verify(plus, key.vk, pis) == O.plonk_verify(minus, key.vk, pis) == PAIRING_FAILED
    b.proofs, b.rows, want = bytes(proofs), bytes(rows), bytes(want)
    assert want.count(bytes([PAIRING_FAILED])) == 30 and OFF_H + 64 <= 904
    coop_before = pkg.dbg_plonk_keys_knobs()[0]
    if form == "lanes":
        pkg.set_plonk_keys_params(0)
    try:
        ks = b.key_set(pkg)
        ks.reserve(b.n)
        exact = b.device(ks, torch_dev)
        s0 = ks.state()
        rlc = b.device(ks, torch_dev, flags=pkg.FLAG_RLC)
        s1 = ks.state()
    finally:
        pkg.set_plonk_keys_params(coop_before)
    accepted = [i for i in range(b.n) if want[i] == PAIRING_FAILED and rlc[i] == pkg.ACCEPT]
    assert not accepted, "forged PlonK proofs ACCEPTED under BN254_FLAG_RLC (batch positions): %r" % accepted
    assert rlc == want, diff(rlc, want)
    assert exact == want, diff(exact, want)
    delta = tuple(y - x for x, y in zip(s0, s1))
    assert delta[:3] == (1, 16, 15), delta                        # one joint pass, every granule a group, every planted group failed and the valid one did not
    assert delta[3] == (1 if form == "cooperative" else 0), delta
