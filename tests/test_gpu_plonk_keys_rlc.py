"""BN254_FLAG_RLC on PlonK batches over key lists (csrc/bn254_capi_plonk_keys.hip::pk_run_pass: the pairing checks of a pass batched over its granules, one
cooperative check per group with the group's key, the exact check only behind a failed group) on the GPU.  The status bytes are those of the exact path, so every
case compares bytes; what shows that the joint check ran, and that every group met its own key, are the counters of bn254_plonk_keys_state: passes that ran the joint
check, groups checked, groups failed, cooperative per-proof checks.  The threshold (bn254_set_plonk_rlc_params) is 64 in every case but the one about its default.
One process, every case finite; no case is meant to fault."""
import random
import threading

import pytest

from plonk_keys_common import A, B, C, D, G, PAIRING_FAILED, Batch, check, diff, get_key, shuffled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


@pytest.fixture
def rlc_from_64(pkg):
    """the threshold at 64 for the test and at its value of before afterwards; yields that value (the default)"""
    before = pkg.dbg_plonk_keys_knobs()[1]
    try:
        pkg.set_plonk_rlc_params(64)
        yield before
    finally:
        pkg.set_plonk_rlc_params(before)


def _delta(a, b):
    return tuple(y - x for x, y in zip(a, b))


def _valid_items(pkg, keys, counts, skip=0):
    """(position, proof number) for the first counts[p] ACCEPTed proofs of every key behind its first `skip`, shuffled"""
    items = []
    for p, (k, c) in enumerate(zip(keys, counts)):
        items += [(p, j) for j in k.numbers(lambda s: s == pkg.ACCEPT)[skip:skip + c]]
    random.Random(11).shuffle(items)
    return items


def test_all_valid_every_group_meets_its_own_key(pkg, O, torch_dev, rlc_from_64):
    """200 proofs of A, 130 of B and 64 of C, all valid, shuffled: 4 + 3 + 1 granules, the eight groups in two cooperative wavefronts with three keys in one of
    them.  All ACCEPT, one joint pass over eight groups and NO failed group: a group checked against another key's tables fails, is repaired by the exact check and
    shows in no status byte -- only in this counter.  The exact check does not run, so the count of cooperative per-proof checks stays too."""
    kl = [get_key(pkg, s) for s in (A, B, C)]
    b = Batch(kl, _valid_items(pkg, kl, [200, 130, 64]))
    assert b.slots() == 8 * G
    ks = b.key_set(pkg)
    ks.reserve(b.n)
    for run in (lambda: b.device(ks, torch_dev, flags=pkg.FLAG_RLC), lambda: b.host(ks, flags=pkg.FLAG_RLC)):
        s0 = ks.state()
        got = run()
        assert got == bytes([pkg.ACCEPT]) * b.n, diff(got, bytes([pkg.ACCEPT]) * b.n)
        assert _delta(s0, ks.state()) == (1, 8, 0, 0)
    check(pkg, O, b, got, "all valid")


def test_planted_failures(pkg, O, torch_dev, rlc_from_64):
    """The same valid proofs with, planted: one proof that fails in the pairing alone (status 8) among A's; an entry (D) of 64 proofs that are all decided before the
    pairing; an entry (C again) of 40 proofs that all have status 8; 64 accepted proofs of A, with their own inputs, indexed to an entry of their own that names B.
    Bytes: those of the exact path (flag 0), of one single-key call per key, of the oracle on a sample, and of the generator where the proof carries its own key.
    Failed groups: the granules that hold a proof whose final status is 8, counted on the grouping the entry runs (bn254_dbg_g16_keys_group); every planted class
    has a list entry or a key's run of its own, so the count does not depend on the order of a key's proofs inside its run."""
    a, bk, c, d = (get_key(pkg, s) for s in (A, B, C, D))
    kl = [a, bk, c, d, c, bk]
    items = _valid_items(pkg, kl[:3], [199, 130, 64])
    owner = [kl[p] for p, _ in items]
    planted = [(0, a.numbers(lambda s: s == PAIRING_FAILED)[0])]
    planted += [(3, j) for j in d.numbers(lambda s: s not in (pkg.ACCEPT, PAIRING_FAILED))[:64]]
    planted += [(4, j) for j in c.numbers(lambda s: s == PAIRING_FAILED)[:40]]
    powner = [kl[p] for p, _ in planted]
    swapped = [(5, j) for j in a.numbers(lambda s: s == pkg.ACCEPT)[300:364]]
    assert len(planted) == 105 and len(swapped) == 64
    items, owner = items + planted + swapped, owner + powner + [a] * 64
    order = list(range(len(items)))
    random.Random(12).shuffle(order)
    b = Batch(kl, [items[i] for i in order], owner=[owner[i] for i in order])
    is_swapped = [order[i] >= len(items) - 64 for i in range(b.n)]
    assert b.slots() == (4 + 3 + 1 + 1 + 1 + 1) * G
    ks = b.key_set(pkg)
    ks.reserve(b.n)
    exact = b.device(ks, torch_dev)
    s0 = ks.state()
    got = b.device(ks, torch_dev, flags=pkg.FLAG_RLC)
    s1 = ks.state()
    host = b.host(ks, flags=pkg.FLAG_RLC)
    s2 = ks.state()
    assert got == exact, "BN254_FLAG_RLC against the exact path: " + diff(got, exact)
    assert host == exact, "host entry: " + diff(host, exact)
    per_key = b.per_key_calls()
    assert got == per_key, "against one call per key: " + diff(got, per_key)
    assert b.oracle_sample(O, got) >= 4
    for i in range(b.n):
        p, j = b.items[i]
        if not is_swapped[i]:
            assert got[i] == kl[p].exp[j], i
        else:
            assert got[i] != pkg.ACCEPT, i
    assert got.count(bytes([pkg.ACCEPT])) == 199 + 130 + 64
    # the groups that must fail, on the host compile of the grouping
    s2p, gk, n_slots = pkg.dbg_keys_group(b.index, len(kl), device=-1)
    assert n_slots == b.slots()
    failing = {s // G for s in range(n_slots) if s2p[s] < b.n and got[s2p[s]] == PAIRING_FAILED}
    pending = {s // G for s in range(n_slots) if s2p[s] < b.n and got[s2p[s]] in (pkg.ACCEPT, PAIRING_FAILED)}
    assert len(failing) >= 2 and len(pending - failing) >= 2
    assert any(gk[g] == 3 for g in range(n_slots // G)) and all(gk[g] != 3 for g in pending)      # D's granule: every proof decided before the pairing
    for s_a, s_b in ((s0, s1), (s1, s2)):
        assert _delta(s_a, s_b) == (1, n_slots // G, len(failing), 1), (s0, s1, s2, sorted(failing))


def test_two_chains(pkg, O, torch_dev, rlc_from_64):
    """6450 proofs, seven of eight valid, in two chains with the cut inside a key's run: two joint passes per call, the bytes of the exact path, both entries"""
    kl = [get_key(pkg, s) for s in (A, C, D)]
    b = Batch(kl, shuffled([2100, 2150, 2200]), proof_stride=1000, input_stride=160)
    plan = pkg.dbg_plonk_keys_plan(b.n, 3, b.slots())
    assert plan["workers"] == 2 and len(plan["pass_first"]) == 2
    ks = b.key_set(pkg)
    ks.reserve(b.n, proof_stride=1000)
    exact = b.device(ks, torch_dev)
    assert exact == b.exp, diff(exact, b.exp)
    s0 = ks.state()
    dev = b.device(ks, torch_dev, flags=pkg.FLAG_RLC)
    s1 = ks.state()
    host = b.host(ks, flags=pkg.FLAG_RLC)
    s2 = ks.state()
    assert dev == exact, "device entry: " + diff(dev, exact)
    assert host == exact, "host entry: " + diff(host, exact)
    for s_a, s_b in ((s0, s1), (s1, s2)):
        dl = _delta(s_a, s_b)
        assert dl[0] == 2 and dl[1] == b.slots() // G and 1 <= dl[2] <= dl[1], dl


def test_default_threshold_leaves_small_passes_exact(pkg, O, torch_dev, rlc_from_64):
    """with the threshold at its default, 300 proofs with the flag: no counter of the joint check moves, the same bytes"""
    assert rlc_from_64 > 300 + 3 * 63
    kl = [get_key(pkg, s) for s in (A, B, C)]
    b = Batch(kl, shuffled([100, 100, 100], seed=3))
    ks = b.key_set(pkg)
    ks.reserve(b.n)
    exact = b.device(ks, torch_dev)
    assert exact == b.exp, diff(exact, b.exp)
    pkg.set_plonk_rlc_params(rlc_from_64)
    s0 = ks.state()
    got = b.device(ks, torch_dev, flags=pkg.FLAG_RLC)
    assert _delta(s0, ks.state())[:3] == (0, 0, 0)
    assert got == exact, diff(got, exact)
    pkg.set_plonk_rlc_params(64)
    got = b.device(ks, torch_dev, flags=pkg.FLAG_RLC)
    assert _delta(s0, ks.state())[0] == 1 and got == exact


def test_two_host_threads_one_with_the_flag(pkg, O, rlc_from_64):
    kl = [get_key(pkg, s) for s in (A, C, D)]
    ks = pkg.PlonkKeySet([k.pvk for k in kl])
    batches = [Batch(kl, shuffled(c, seed=7 + t)) for t, c in enumerate(([700, 700, 600], [600, 650, 750]))]
    ks.reserve(2000)
    out = [None, None]
    s0 = ks.state()

    def run(t):
        out[t] = batches[t].host(ks, flags=pkg.FLAG_RLC if t == 0 else 0)

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert _delta(s0, ks.state())[0] == 1                      # one pass of one call ran the joint check
    for t in range(2):
        assert out[t] is not None
        check(pkg, O, batches[t], out[t], "thread %d" % t)
