"""PlonK batches over many verifying keys in one call (bn254_plonk_verify_batch_keys, include/bn254_verify.h "PlonK batches over many keys") on the GPU.

The definition of correctness is per proof: status[i] is what the single-key entry writes for (proof i, its key) with the key's own input count.  Every case
compares the mixed batch with (a) the generator's expected statuses, (b) one bn254_plonk_verify_batch per key on the same GPU, put back into batch order, and (c)
the CPU oracle O.plonk_verify on a sample that covers every key, every status value present per key and at least three ACCEPTs per key.  A cap keeps a case from
passing on all-failures: the ACCEPT bytes are counted against the generator's, n - n // 8 per key.  Key shapes are (n_public, n_qcp, log2 size); proofs come from
bn254_synth_plonk with every eighth proof invalid, so all six invalid classes occur.  One process, every case finite; no case is meant to fault."""
import array
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

G = 64
MALFORMED = 6
N_KEY = 2400            # proofs generated per class-1 key (cases 1 and 5 take prefixes)


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


class Key:
    def __init__(self, pkg, shape, n):
        self.shape, self.n, self.n_public, self.plen = shape, n, shape[0], 808 + 96 * shape[1]
        seed = 0x504B0000 + 4096 * shape[0] + 64 * shape[1] + shape[2]          # its own seed: its own SRS
        self.vk, self.proofs, self.inputs, self.exp = pkg.synth_plonk(seed, shape[0], shape[1], shape[2], n, invalid_every=8, threads=16)
        self.pvk = pkg.PreparedPlonkVk(self.vk)

    def proof(self, j):
        return self.proofs[self.plen * j:self.plen * (j + 1)]

    def row(self, j):
        return self.inputs[32 * self.n_public * j:32 * self.n_public * (j + 1)]


@pytest.fixture(scope="module")
def key(pkg):
    """shape -> its key and proofs: generated once and never changed"""
    cache = {}

    def get(shape, n=N_KEY):
        if shape not in cache:
            cache[shape] = Key(pkg, shape, n)
        assert cache[shape].n >= n
        return cache[shape]

    yield get
    for k in cache.values():
        k.pvk.close()


class Batch:
    """items: (position in the key list, proof number of that position's key), in batch order.  key_list: position -> key (a key may occur twice)."""

    def __init__(self, key_list, items, proof_stride=None, input_stride=None, owner=None):
        self.key_list, self.items = key_list, items
        self.owner = owner or [key_list[p] for p, _ in items]                      # the key whose proof (and inputs) item i carries; differs from its list entry in case 4
        self.plen = key_list[0].plen
        self.proof_stride = self.plen if proof_stride is None else proof_stride
        self.input_stride = 32 * max(k.n_public for k in key_list) if input_stride is None else input_stride
        self.index = [p for p, _ in items]
        junk = bytes((37 * i + 11) & 0xFF for i in range(self.proof_stride - self.plen))
        self.proofs = b"".join(o.proof(j) + junk for o, (_, j) in zip(self.owner, items))
        self.rows = b"".join(o.row(j).ljust(self.input_stride, b"\xa5") for o, (_, j) in zip(self.owner, items))      # bytes behind a key's inputs are never read
        self.exp = bytes(key_list[p].exp[j] for p, j in items) if owner is None else None
        self.n = len(items)

    def key_set(self, pkg):
        return pkg.PlonkKeySet([k.pvk for k in self.key_list])

    def host(self, ks, flags=0):
        return ks.verify_batch(self.index, self.proofs, self.rows, proof_stride=self.proof_stride, input_stride=self.input_stride, flags=flags)

    def device(self, ks, torch_dev, flags=0, index=None):
        torch, dev = torch_dev
        idx = array.array("I", self.index if index is None else index)
        d_x = torch.frombuffer(bytearray(idx.tobytes()), dtype=torch.uint8).to(dev)
        d_p = torch.frombuffer(bytearray(self.proofs), dtype=torch.uint8).to(dev)
        d_i = torch.frombuffer(bytearray(self.rows or b"\0"), dtype=torch.uint8).to(dev)
        d_s = torch.full((self.n,), 0xEE, dtype=torch.uint8, device=dev)
        ks.verify_batch_device(d_x.data_ptr(), d_p.data_ptr(), d_i.data_ptr() if self.input_stride else None, d_s.data_ptr(), self.n, proof_stride=self.proof_stride,
                               input_stride=self.input_stride, device=dev.index, stream=torch.cuda.current_stream(dev).cuda_stream, flags=flags)
        return bytes(d_s.cpu().numpy().tobytes())

    def per_key_calls(self):
        """(b): what a caller does today -- one bn254_plonk_verify_batch per key on that key's proofs -- put back into batch order"""
        out = bytearray(self.n)
        for k in {id(k): k for k in self.key_list}.values():
            mine = [i for i, (p, _) in enumerate(self.items) if self.key_list[p] is k]
            if not mine:
                continue
            st = k.pvk.verify_batch(b"".join(self.owner[i].proof(self.items[i][1]) for i in mine), b"".join(self.owner[i].row(self.items[i][1]) for i in mine), n=len(mine),
                                    proof_stride=self.plen, n_public=k.n_public)
            for i, s in zip(mine, st):
                out[i] = s
        return bytes(out)

    def oracle_sample(self, O, got):
        """(c): per key, the first proof of every status value present and the first three ACCEPTs"""
        checked = 0
        for k in {id(k): k for k in self.key_list}.values():
            mine = [i for i, (p, _) in enumerate(self.items) if self.key_list[p] is k]
            want, accepts = set(), 0
            for i in mine:
                s = got[i]
                if s in want and not (s == 1 and accepts < 3):
                    continue
                want.add(s)
                accepts += s == 1
                o, j = self.owner[i], self.items[i][1]
                ref = O.plonk_verify(o.proof(j), k.vk, [o.row(j)[32 * t:32 * t + 32] for t in range(k.n_public)])
                assert ref == s, "proof %d (key %r): got %d, oracle %d" % (i, k.shape, s, ref)
                checked += 1
            if self.exp is not None and mine:
                assert accepts >= min(3, sum(self.exp[i] == 1 for i in mine))
        return checked


def _diff(got, want):
    d = [i for i in range(len(want)) if got[i] != want[i]]
    return "%d of %d status bytes differ, first at %d: got %d, expected %d" % (len(d), len(want), d[0], got[d[0]], want[d[0]]) if d else ""


def _check(pkg, O, b, got, what, full_prefix=False):
    assert len(got) == b.n
    assert got == b.exp, "%s against the generator: %s" % (what, _diff(got, b.exp))
    assert got.count(bytes([pkg.ACCEPT])) == b.exp.count(bytes([pkg.ACCEPT]))
    if full_prefix:       # every key contributes the proofs [0, n_k) of its stream: every eighth is invalid
        counts = {}
        for p, _ in b.items:
            counts[id(b.key_list[p])] = counts.get(id(b.key_list[p]), 0) + 1
        assert got.count(bytes([pkg.ACCEPT])) == sum(c - c // 8 for c in counts.values())
    per_key = b.per_key_calls()
    assert got == per_key, "%s against one call per key: %s" % (what, _diff(got, per_key))
    assert b.oracle_sample(O, got) >= len({id(k) for k in b.key_list if any(b.key_list[p] is k for p, _ in b.items)})


def _shuffled(key_list, counts, seed=1):
    items = [(p, j) for p, c in enumerate(counts) for j in range(c)]
    random.Random(seed).shuffle(items)
    return items


def test_parity_class_1(pkg, O, torch_dev, key):
    """6450 proofs of three keys with one commitment each: two chains, the cut inside a key's run; junk behind the proofs and behind the narrower input rows"""
    kl = [key((2, 1, 26)), key((1, 1, 10)), key((5, 1, 12))]
    b = Batch(kl, _shuffled(kl, [2100, 2150, 2200]), proof_stride=1000, input_stride=160)
    plan = pkg.dbg_plonk_keys_plan(b.n, 3, sum((c + G - 1) // G * G for c in (2100, 2150, 2200)))
    assert plan["workers"] == 2 and len(plan["pass_first"]) == 2          # two chains; the second starts inside the second key's run (2112 + 2176 > 3264 > 2112)
    ks = b.key_set(pkg)
    got = b.host(ks)
    _check(pkg, O, b, got, "host buffers", full_prefix=True)
    dev = b.device(ks, torch_dev)
    assert dev == got, "device entry: " + _diff(dev, got)


@pytest.mark.parametrize("shapes", [[(1, 0, 10), (0, 0, 3), (3, 0, 8)], [(3, 2, 20), (2, 2, 9)], [(5, 8, 28), (1, 8, 12)]], ids=["class0", "class2", "class8"])
def test_other_commitment_classes(pkg, O, torch_dev, key, shapes):
    kl = [key(s, 700) for s in shapes]
    b = Batch(kl, _shuffled(kl, [700] * len(kl), seed=2))
    ks = b.key_set(pkg)
    got = b.host(ks)
    _check(pkg, O, b, got, "host buffers", full_prefix=True)
    dev = b.device(ks, torch_dev)
    assert dev == got, "device entry: " + _diff(dev, got)


def test_granule_edges(pkg, O, torch_dev, key):
    a, c, d = key((2, 1, 26)), key((1, 1, 10)), key((5, 1, 12))
    two = [a, c]
    cases = [("n = 1", Batch(two, [(1, 5)]))]
    for ca, cc in ((63, 1), (64, 1), (65, 64), (1, 1)):
        cases.append(("runs of %d and %d" % (ca, cc), Batch(two, _shuffled(two, [ca, cc], seed=ca))))
    cases.append(("an entry without proofs", Batch([a, d, c], [(0, j) for j in range(70)] + [(2, j) for j in range(9)])))
    twice = [a, c, a]
    cases.append(("a handle listed twice", Batch(twice, [(0 if j % 2 else 2, j) for j in range(100)] + [(1, j) for j in range(30)])))
    eight = [a, c, d, a, c, d, a, c]
    cases.append(("eight entries, three handles, one proof each", Batch(eight, [(p, 8 + p) for p in range(8)])))
    for what, b in cases:
        ks = b.key_set(pkg)
        got = b.host(ks)
        _check(pkg, O, b, got, what)
        dev = b.device(ks, torch_dev)
        assert dev == got, what + ", device entry: " + _diff(dev, got)


def test_the_key_is_the_granules(pkg, O, torch_dev, key):
    """64 accepted proofs of key A, with their own inputs, indexed to key B of the same class and width, among A's and B's own proofs: each is judged by B"""
    a, bkey = key((2, 1, 26)), key((2, 1, 9))
    acc = [j for j in range(a.n) if a.exp[j] == pkg.ACCEPT][100:164]
    kl = [a, bkey]
    items = [(0, j) for j in range(90)] + [(1, j) for j in range(90)] + [(1, j) for j in acc]
    owner = [a] * 90 + [bkey] * 90 + [a] * 64
    order = list(range(len(items)))
    random.Random(4).shuffle(order)
    b = Batch(kl, [items[i] for i in order], owner=[owner[i] for i in order])
    ks = b.key_set(pkg)
    got = b.host(ks)
    dev = b.device(ks, torch_dev)
    assert dev == got, "device entry: " + _diff(dev, got)
    per_key = b.per_key_calls()                       # (b): the swapped proofs go to key B's own call with their own inputs
    assert got == per_key, "against one call per key: " + _diff(got, per_key)
    assert b.oracle_sample(O, got) >= 2               # (c)
    swapped = [i for i, t in enumerate(order) if t >= 180]
    assert len(swapped) == 64
    for i, t in enumerate(order):
        if t < 180:
            assert got[i] == kl[items[t][0]].exp[items[t][1]], i
    for i in swapped:
        j = b.items[i][1]
        ref = O.plonk_verify(a.proof(j), bkey.vk, [a.row(j)[32 * t:32 * t + 32] for t in range(2)])
        assert got[i] == ref and got[i] != pkg.ACCEPT, (i, got[i], ref)
    assert got.count(bytes([pkg.ACCEPT])) == sum(kl[items[t][0]].exp[items[t][1]] == pkg.ACCEPT for t in range(180))


def test_one_pass_larger(pkg, O, torch_dev, key):
    """12 000 proofs over five keys: the single-pass form of the plan; with BN254_FLAG_RLC the same bytes (the flag is accepted and ignored)"""
    kl = [key((2, 1, 26)), key((1, 1, 10)), key((5, 1, 12)), key((2, 1, 9)), key((3, 1, 14))]
    b = Batch(kl, _shuffled(kl, [N_KEY] * 5, seed=5))
    plan = pkg.dbg_plonk_keys_plan(b.n, 5, 5 * ((N_KEY + G - 1) // G * G))
    assert plan["workers"] == 1 and len(plan["pass_first"]) == 1
    ks = b.key_set(pkg)
    got = b.device(ks, torch_dev)
    _check(pkg, O, b, got, "device entry", full_prefix=True)
    rlc = b.device(ks, torch_dev, flags=pkg.FLAG_RLC)
    assert rlc == got, "BN254_FLAG_RLC: " + _diff(rlc, got)


def test_device_entry_with_a_bad_index(pkg, torch_dev, key):
    kl = [key((2, 1, 26)), key((1, 1, 10))]
    b = Batch(kl, _shuffled(kl, [150, 150], seed=6))
    index = list(b.index)
    bad = (0, 77, 299)
    for i, v in zip(bad, (2, 0xFFFFFFFF, 1000)):
        index[i] = v
    got = b.device(b.key_set(pkg), torch_dev, index=index)
    for i in range(b.n):
        assert got[i] == (MALFORMED if i in bad else b.exp[i]), i
    assert got.count(bytes([pkg.ACCEPT])) == sum(b.exp[i] == pkg.ACCEPT for i in range(b.n) if i not in bad)


def test_two_host_threads_on_one_set(pkg, O, key):
    kl = [key((2, 1, 26)), key((1, 1, 10)), key((5, 1, 12))]
    ks = pkg.PlonkKeySet([k.pvk for k in kl])
    batches = [Batch(kl, _shuffled(kl, c, seed=7 + t)) for t, c in enumerate(([700, 700, 600], [600, 650, 750]))]
    ks.reserve(2000)
    out = [None, None]

    def run(t):
        out[t] = batches[t].host(ks)

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for t in range(2):
        assert out[t] is not None and out[t].count(bytes([pkg.ACCEPT])) > 1500
        _check(pkg, O, batches[t], out[t], "thread %d" % t, full_prefix=True)


def test_reserve_then_call_and_single_key_calls_between(pkg, O, torch_dev, key):
    """the member's own state and the set's do not disturb each other"""
    kl = [key((2, 1, 26)), key((2, 1, 9))]
    b = Batch(kl, _shuffled(kl, [500, 300], seed=9))
    ks = b.key_set(pkg)
    ks.reserve(b.n, proof_stride=b.proof_stride)
    first = b.device(ks, torch_dev)
    _check(pkg, O, b, first, "device entry after reserve", full_prefix=True)
    a = kl[0]
    assert a.pvk.verify_batch(a.proofs[:a.plen * 300], a.inputs[:64 * 300], n=300, proof_stride=a.plen) == a.exp[:300]
    again = b.device(ks, torch_dev)
    assert again == first
    assert a.pvk.verify_batch(a.proofs[:a.plen * 300], a.inputs[:64 * 300], n=300, proof_stride=a.plen) == a.exp[:300]
    assert first.count(bytes([pkg.ACCEPT])) == b.exp.count(bytes([pkg.ACCEPT])) > 600
