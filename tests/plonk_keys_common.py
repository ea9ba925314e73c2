"""What the tests of the PlonK batches over key lists in their cooperative and BN254_FLAG_RLC forms share (tests/test_gpu_plonk_keys_coop.py, _rlc.py): the four key
shapes with one commitment of tests/test_gpu_plonk_keys.py, each with its own seed and SRS and 2400 proofs of which every eighth is invalid -- generated once per
process and never changed --, batches composed from them, and the three-way check of that file restated: the generator's statuses, one single-key call per key,
and the CPU oracle on a sample per key."""
import array
import random

G = 64
N_KEY = 2400
A, B, C, D = (2, 1, 26), (2, 1, 9), (1, 1, 10), (5, 1, 12)      # (n_public, n_qcp, log2 size)
PAIRING_FAILED = 8
_KEYS = {}


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

    def numbers(self, pred):
        """proof numbers whose expected status satisfies pred, in order"""
        return [j for j in range(self.n) if pred(self.exp[j])]


def get_key(pkg, shape):
    if shape not in _KEYS:
        _KEYS[shape] = Key(pkg, shape, N_KEY)
    return _KEYS[shape]


class Batch:
    """items: (position in the key list, proof number), in batch order.  key_list: position -> key (a key may occur twice).  owner: the key whose proof and inputs
    item i carries, where that is not its list entry (then the generator has no expectation for the batch)."""

    def __init__(self, key_list, items, proof_stride=None, input_stride=None, owner=None):
        self.key_list, self.items = key_list, items
        self.owner = owner or [key_list[p] for p, _ in items]
        self.plen = key_list[0].plen
        self.proof_stride = self.plen if proof_stride is None else proof_stride
        self.input_stride = 32 * max(k.n_public for k in key_list) if input_stride is None else input_stride
        self.index = [p for p, _ in items]
        junk = bytes((37 * i + 11) & 0xFF for i in range(self.proof_stride - self.plen))
        self.proofs = b"".join(o.proof(j) + junk for o, (_, j) in zip(self.owner, items))
        self.rows = b"".join(o.row(j).ljust(self.input_stride, b"\xa5") for o, (_, j) in zip(self.owner, items))      # bytes behind a key's inputs are never read
        self.exp = bytes(key_list[p].exp[j] for p, j in items) if owner is None else None
        self.n = len(items)
        self._dev = None

    def key_set(self, pkg):
        return pkg.PlonkKeySet([k.pvk for k in self.key_list])

    def slots(self):
        """slots of the batch's grouping: every list entry's proofs rounded up to a granule"""
        counts = {}
        for p in self.index:
            counts[p] = counts.get(p, 0) + 1
        return sum((c + G - 1) // G * G for c in counts.values())

    def host(self, ks, flags=0):
        return ks.verify_batch(self.index, self.proofs, self.rows, proof_stride=self.proof_stride, input_stride=self.input_stride, flags=flags)

    def device(self, ks, torch_dev, flags=0):
        torch, dev = torch_dev
        if self._dev is None:
            idx = array.array("I", self.index)
            self._dev = tuple(torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to(dev) for b in (idx.tobytes(), self.proofs, self.rows))
        d_x, d_p, d_i = self._dev
        d_s = torch.full((self.n,), 0xEE, dtype=torch.uint8, device=dev)
        ks.verify_batch_device(d_x.data_ptr(), d_p.data_ptr(), d_i.data_ptr() if self.input_stride else None, d_s.data_ptr(), self.n, proof_stride=self.proof_stride,
                               input_stride=self.input_stride, device=dev.index, stream=torch.cuda.current_stream(dev).cuda_stream, flags=flags)
        return bytes(d_s.cpu().numpy().tobytes())

    def per_key_calls(self):
        """one bn254_plonk_verify_batch per key on that key's proofs, put back into batch order"""
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
        """per key, the first proof of every status value present and the first three ACCEPTs"""
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


def diff(got, want):
    d = [i for i in range(len(want)) if got[i] != want[i]]
    return "%d of %d status bytes differ, first at %d: got %d, expected %d" % (len(d), len(want), d[0], got[d[0]], want[d[0]]) if d else ""


def check(pkg, O, b, got, what):
    """the generator's statuses (with the ACCEPT count as the cap against all-failures), one single-key call per key, the oracle on a sample per key"""
    assert len(got) == b.n
    assert got == b.exp, "%s against the generator: %s" % (what, diff(got, b.exp))
    assert got.count(bytes([pkg.ACCEPT])) == b.exp.count(bytes([pkg.ACCEPT]))
    per_key = b.per_key_calls()
    assert got == per_key, "%s against one call per key: %s" % (what, diff(got, per_key))
    assert b.oracle_sample(O, got) >= len({id(b.key_list[p]) for p in b.index})


def shuffled(counts, seed=1):
    items = [(p, j) for p, c in enumerate(counts) for j in range(c)]
    random.Random(seed).shuffle(items)
    return items
