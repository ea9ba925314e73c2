"""Groth16 batches over many verifying keys in one call (bn254_groth16_verify_batch_keys, include/bn254_verify.h "Batches over many keys") on the GPU.

The definition of correctness is per proof: status[i] is what the single-key entry writes for (proof i, its key) without the RLC flag.  Every case compares the
mixed batch with (a) the generator's expected statuses, (b) per-key bn254_groth16_verify_batch calls on the same GPU, and where it says so (c) the CPU oracle,
O.groth16_verify_many(proof, 256, vk_of_that_proof, inputs, n_public, 1).  One process, every case finite; no case is meant to fault."""
import array
import random

import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
G = 64                      # csrc/bn254_keys.h: G16_KEYS_GRANULE
NO_K = (1 << 64) - 1        # bn254_groth16_vk_num_public of a key without K points


class Key:
    """A synthetic key with its own proofs: (vk bytes, mode, n_public, proofs, inputs, expected)"""

    def __init__(self, pkg, seed, n_public, n, mode=0, invalid_every=37, threads=16):
        self.vk, self.proofs, self.inputs, self.exp = pkg.synth_groth16(seed, n_public, n, invalid_every=invalid_every, agree=True, threads=threads)
        self.n_public, self.n, self.mode = n_public, n, mode
        self.pvk = pkg.PreparedVk(self.vk, mode)

    def proof(self, j):
        return self.proofs[256 * j:256 * j + 256]

    def row(self, j):
        return self.inputs[32 * self.n_public * j:32 * self.n_public * (j + 1)]


class Mixed:
    """Proofs of several keys shuffled into one batch: entries (key number in `keys`, proof number of that key)."""

    def __init__(self, keys, entries=None, seed=1, key_list=None):
        self.keys = keys
        self.key_list = list(range(len(keys))) if key_list is None else key_list      # list entry -> key number (a handle may occur twice)
        if entries is None:
            entries = [(k, j) for k, key in enumerate(keys) for j in range(key.n)]
            random.Random(seed).shuffle(entries)
        self.entries = entries
        self.stride = 32 * max([k.n_public for k in keys] + [0])
        first_entry = {}
        for e, k in enumerate(self.key_list):
            first_entry.setdefault(k, e)
        self.index = [first_entry[k] for k, _ in entries]
        self.proofs = b"".join(keys[k].proof(j) for k, j in entries)
        self.rows = b"".join(keys[k].row(j).ljust(self.stride, b"\xa5") for k, j in entries)          # what lies behind a key's inputs in its row is never read
        self.exp = bytes(keys[k].exp[j] for k, j in entries)

    def key_set(self, pkg):
        return pkg.KeySet([self.keys[k].pvk for k in self.key_list])

    def run(self, ks, index=None, proofs=None, rows=None, **kw):
        return ks.verify_batch(self.index if index is None else index, self.proofs if proofs is None else proofs, self.rows if rows is None else rows,
                               input_stride=self.stride, **kw)

    def per_key_calls(self, flags=0, proofs_of=None, compressed=False):
        """what a caller does today: one bn254_groth16_verify_batch per key on that key's proofs, put back into batch order"""
        out = bytearray(len(self.entries))
        for k, key in enumerate(self.keys):
            pos = [i for i, (kk, _) in enumerate(self.entries) if kk == k]
            if not pos:
                continue
            rec = 128 if compressed else 256
            src = proofs_of if proofs_of is not None else self.proofs
            pr = b"".join(src[rec * i:rec * i + rec] for i in pos)
            ins = b"".join(self.rows[self.stride * i:self.stride * i + 32 * key.n_public] for i in pos)
            st = key.pvk.verify_batch(pr, ins, n=len(pos), n_public=key.n_public, flags=flags, compressed=compressed)
            for i, s in zip(pos, st):
                out[i] = s
        return bytes(out)

    def oracle(self, O, i):
        k, j = self.entries[i]
        key = self.keys[k]
        return O.groth16_verify_many(self.proofs[256 * i:256 * i + 256], 256, key.vk, self.rows[self.stride * i:self.stride * i + 32 * key.n_public], key.n_public, 1,
                                     O.MODE_GNARK if key.mode else O.MODE_REFERENCE)[0]


@pytest.fixture(scope="module")
def twelve(pkg):
    """twelve keys: n_public 0, 1, 2, 5, 8, 16 in both modes, 1 700 .. 2 250 proofs each (23 700 in total), every 37th invalid"""
    keys = [Key(pkg, 0x4B0000 + 16 * m + p, p, 1700 + 50 * i, mode=m) for i, (p, m) in enumerate((p, m) for m in (pkg.VK_REFERENCE, pkg.VK_GNARK) for p in (0, 1, 2, 5, 8, 16))]
    yield keys
    for k in keys:
        k.pvk.close()


def test_grouping_kernels(pkg):
    """k_keys_count / k_keys_scan / k_keys_place against the conditions the host compile is held to (tests/test_multikey_cpu.py): LDS-privatised and global counters,
    one key, every proof its own key, a skewed distribution"""
    from test_multikey_cpu import _check_grouping
    rng = random.Random(12)
    for n in (1, G - 1, G + 1, 100003):
        _check_grouping(pkg, [0] * n, 1, device=0)
        _check_grouping(pkg, [rng.randrange(257) for _ in range(n)], 257, device=0)
        _check_grouping(pkg, [rng.choice([0, 77, 65535, 40000]) if i % 3 else rng.randrange(65536) for i in range(n)], 65536, device=0)
        _check_grouping(pkg, [5 if i % 2 else rng.randrange(9000) for i in range(n)], 9000, device=0)
    perm = list(range(65536)); rng.shuffle(perm)
    _check_grouping(pkg, perm, 65536, device=0)


def test_parity_twelve_keys(pkg, O, twelve):
    mx = Mixed(twelve, seed=11)
    assert 20000 <= len(mx.entries) <= 40000
    for k, key in enumerate(twelve):
        assert any(s != pkg.ACCEPT for s in key.exp), k
    ks = mx.key_set(pkg)
    st = mx.run(ks)
    bad = [i for i in range(len(st)) if st[i] != mx.exp[i]]
    assert st == mx.exp, ("generator", len(bad), [(i, mx.entries[i], st[i], mx.exp[i]) for i in bad[:10]])
    assert st == mx.per_key_calls()
    # the oracle on a sample that covers every key and, per key, every status value present
    sample, seen = [], set()
    for i, (k, j) in enumerate(mx.entries):
        if (k, st[i]) not in seen or (st[i] == pkg.ACCEPT and sum(1 for s in sample if mx.entries[s][0] == k) < 3):
            seen.add((k, st[i])); sample.append(i)
    assert len(sample) >= 48 and {mx.entries[i][0] for i in sample} == set(range(12)) and {st[i] for i in sample} == set(st)
    for i in sample:
        assert st[i] == mx.oracle(O, i), (i, mx.entries[i])


def test_the_index_is_honoured(pkg, O):
    """valid proofs of key a submitted under key b (same n_public) are what the oracle says for (proof, key b) -- not ACCEPT -- while the same proofs under key a in
    the same batch are accepted: a kernel that read granule 0's key everywhere passes every one-key batch and fails here"""
    a, b = Key(pkg, 0x4B1001, 2, 100, invalid_every=0), Key(pkg, 0x4B1002, 2, 100, invalid_every=0)
    mx = Mixed([a, b], seed=3)
    crossed = [1 - k for k in mx.index]
    index = mx.index + crossed
    st = mx.run(pkg.KeySet([a.pvk, b.pvk]), index, mx.proofs + mx.proofs, mx.rows + mx.rows)
    n = len(mx.entries)
    assert st[:n] == bytes([pkg.ACCEPT]) * n
    keys = [a, b]
    for i in range(n):
        want = O.groth16_verify_many(mx.proofs[256 * i:256 * i + 256], 256, keys[crossed[i]].vk, mx.rows[64 * i:64 * i + 64], 2, 1)[0] if i < 12 else pkg.REJECT
        assert st[n + i] == want and want != pkg.ACCEPT, i
    a.pvk.close(); b.pvk.close()


def test_shapes_one_key_one_proof_less_than_a_granule(pkg, twelve):
    key = twelve[2]
    one = pkg.KeySet([key.pvk])
    n = key.n
    assert one.verify_batch([0] * n, key.proofs, key.inputs) == key.pvk.verify_batch(key.proofs, key.inputs) == key.exp
    for m in (1, G - 1):
        assert one.verify_batch([0] * m, key.proofs[:256 * m], key.inputs[:64 * m]) == key.exp[:m]
    mx = Mixed(twelve, entries=[(k, j) for j in range(3) for k in range(12)][:G - 1])          # fewer proofs than one granule, over twelve keys
    assert mx.run(mx.key_set(pkg)) == mx.exp


def test_shapes_128_one_input_keys(pkg):
    """128 one-input keys (84 MB of byte-window tables in one allocation) with 1 .. 300 proofs each"""
    rng = random.Random(5)
    keys = [Key(pkg, 0x4B2000 + i, 1, rng.choice([1, 2, 63, 64, 65, 300, rng.randrange(1, 301)]), invalid_every=7, threads=4) for i in range(128)]
    mx = Mixed(keys, seed=6)
    st = mx.run(mx.key_set(pkg))
    assert st == mx.exp
    for k in keys:
        k.pvk.close()


def test_shapes_most_of_a_1000_entry_list_unused(pkg, twelve):
    """a list of 1000 entries that names the same few handles again and again; the proofs use entries spread over it"""
    rng = random.Random(8)
    key_list = [rng.choice([1, 2, 4]) for _ in range(1000)]
    ks = pkg.KeySet([twelve[k].pvk for k in key_list])
    entries = [(k, j) for k in (1, 2, 4) for j in range(400)]
    rng.shuffle(entries)
    mx = Mixed(twelve, entries=entries)
    where = {k: [e for e, kk in enumerate(key_list) if kk == k] for k in (1, 2, 4)}
    index = [rng.choice(where[k][:3] + where[k][-3:]) for k, _ in entries]
    assert mx.run(ks, index) == mx.exp


def _big(pkg, counts, seed):
    keys = [Key(pkg, seed + i, 2, c, invalid_every=16) for i, c in enumerate(counts)]
    # a shuffle of a million Python tuples is slow and adds nothing: interleave the keys' proofs in runs of pseudo-random length instead
    rng = random.Random(seed)
    nxt = [0] * len(keys)
    entries = []
    while any(nxt[k] < keys[k].n for k in range(len(keys))):
        k = rng.randrange(len(keys))
        m = min(rng.choice([1, 3, 40, 700]), keys[k].n - nxt[k])
        entries.extend((k, j) for j in range(nxt[k], nxt[k] + m))
        nxt[k] += m
    return keys, entries


def _check_big(pkg, O, keys, entries):
    index = array.array("I", [k for k, _ in entries])
    proofs = bytearray(256 * len(entries)); rows = bytearray(64 * len(entries)); exp = bytearray(len(entries))
    for i, (k, j) in enumerate(entries):
        proofs[256 * i:256 * i + 256] = keys[k].proof(j); rows[64 * i:64 * i + 64] = keys[k].row(j); exp[i] = keys[k].exp[j]
    st = pkg.KeySet([k.pvk for k in keys]).verify_batch(index, proofs, rows, input_stride=64)
    assert len(st) == len(entries) and st == bytes(exp)
    assert set(st) == {0, 1, 2, 3, 4}
    step = len(entries) // 40
    for i in list(range(0, len(entries), step)) + [len(entries) - 1]:
        k, j = entries[i]
        assert st[i] == O.groth16_verify_many(keys[k].proof(j), 256, keys[k].vk, keys[k].row(j), 2, 1)[0], i
    for k in keys:
        k.pvk.close()


def test_shapes_above_65536_slots(pkg, O):
    """two sub-batches: the cut falls inside a key's run"""
    keys, entries = _big(pkg, [50000, 30000, 9001], 0x4B3000)
    _check_big(pkg, O, keys, entries)


def test_shapes_above_2_to_the_20_slots(pkg, O):
    """three keys, 2^20 + 777 proofs: two workspace chunks, the chunk boundary inside a key's run"""
    keys, entries = _big(pkg, [600000, 300000, (1 << 20) + 777 - 900000], 0x4B4000)
    _check_big(pkg, O, keys, entries)


def test_flags(pkg, twelve):
    sub = [twelve[i] for i in (0, 2, 4, 7, 11)]
    entries = [(k, j) for k in range(len(sub)) for j in range(300)]
    random.Random(4).shuffle(entries)
    mx = Mixed(sub, entries=entries)
    ks = mx.key_set(pkg)
    plain = mx.per_key_calls()
    # RLC: accepted and ignored, the bytes of the exact path
    assert mx.run(ks, flags=pkg.FLAG_RLC) == plain == mx.exp
    # strict scalars: some inputs >= r (x + r is the same input mod r: the proof stays valid for the default policy and becomes NOT_MEMBER under the flag)
    rows = bytearray(mx.rows)
    hit = 0
    for i, (k, j) in enumerate(entries):
        if sub[k].n_public and i % 5 == 0:
            off = mx.stride * i + 32 * (i % sub[k].n_public)
            x = int.from_bytes(rows[off:off + 32], "big")
            if x + R < 1 << 256:
                rows[off:off + 32] = (x + R).to_bytes(32, "big"); hit += 1
    assert hit > 100
    strict = Mixed(sub, entries=entries); strict.rows = bytes(rows)
    want = strict.per_key_calls(flags=pkg.FLAG_STRICT_SCALARS)
    assert want.count(bytes([pkg.ERR_NOT_MEMBER])) >= hit
    assert mx.run(ks, rows=rows, flags=pkg.FLAG_STRICT_SCALARS) == want
    assert mx.run(ks, rows=rows) == strict.per_key_calls() == mx.exp
    # compressed records; a record that does not decompress is MALFORMED
    comp = bytearray(b"".join(pkg.compress_proof(mx.proofs[256 * i:256 * i + 256]) if mx.exp[i] not in (2, 3) else bytes(128) for i in range(len(entries))))
    comp[128 * 7:128 * 7 + 32] = b"\xff" * 32
    want = mx.per_key_calls(proofs_of=bytes(comp), compressed=True)
    assert pkg.ERR_MALFORMED in want and pkg.ACCEPT in want
    assert mx.run(ks, proofs=bytes(comp), compressed=True) == want


def test_entries_host_and_device(pkg, twelve):
    import torch
    entries = [(k, j) for k in range(12) for j in range(0, 900, 3)]
    random.Random(9).shuffle(entries)
    mx = Mixed(twelve, entries=entries)
    ks = mx.key_set(pkg)
    n = len(mx.entries)
    host = mx.run(ks)
    assert host == mx.exp
    dev = torch.device("cuda:0")
    ks.reserve(n)
    d_p = torch.frombuffer(bytearray(mx.proofs), dtype=torch.uint8).to(dev); d_r = torch.frombuffer(bytearray(mx.rows), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(dev)
    for bad in ([], [0, 5, 777, n - 1]):
        index = list(mx.index)
        for i in bad:
            index[i] = 12 + i
        d_i = torch.tensor(index, dtype=torch.int64).to(torch.int32).to(dev)
        d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ks.verify_batch_device(d_i.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), n, input_stride=mx.stride, stream=stream.cuda_stream)
        stream.synchronize()
        got = bytes(d_s.cpu().numpy().tobytes())
        want = bytearray(host)
        for i in bad:
            want[i] = pkg.ERR_MALFORMED
        assert got == bytes(want), bad
        if bad:
            with pytest.raises(pkg.Bn254Error):          # the host entry checks the whole vector first
                mx.run(ks, index)


def test_edge_keys_in_a_set(pkg, O, twelve):
    """a key without K points, a zero-input key and a two-input key; records with loader errors (coordinate >= p, C off the curve, B outside G2) mixed in: the
    precedence of tests/test_edge_keys.py, against the oracle"""
    zero = twelve[0]
    two = twelve[2]
    no_k_vk = zero.vk[:288] + (0).to_bytes(4, "big") + zero.vk[292 + 32:]
    no_k = pkg.PreparedVk(no_k_vk)
    assert no_k.n_public == NO_K
    ks = pkg.KeySet([no_k, zero.pvk, two.pvk])
    vks, npub = [no_k_vk, zero.vk, two.vk], [0, 0, 2]
    b_outside = next(two.proof(j) for j in range(two.n) if two.exp[j] == pkg.ERR_NOT_IN_SUBGROUP)
    records = []
    for j in range(40):
        good = two.proof(j) if two.exp[j] == pkg.ACCEPT else two.proof(0)
        big = bytearray(good); big[192:224] = b"\xff" * 32                     # C.x >= p
        offc = bytearray(good); offc[255] ^= 1                                 # C off the curve
        offa = bytearray(good); offa[63] ^= 1                                  # A off the curve
        both = bytearray(b_outside); both[255] ^= 1                            # B outside G2 and C off the curve: B's error comes first
        records += [(good, j), (bytes(big), j), (bytes(offc), j), (bytes(offa), j), (b_outside, j), (bytes(both), j)]
    index, proofs, rows, want = [], b"", b"", bytearray()
    for r, (rec, j) in enumerate(records):
        for e in range(3):
            ins = two.row(j)[:32 * npub[e]]
            index.append(e); proofs += rec; rows += two.row(j)
            want.append(O.groth16_verify_many(rec, 256, vks[e], ins, npub[e], 1)[0] if r < 18 or e == 2 and r < 60 else 0xFF)
    st = ks.verify_batch(index, proofs, rows)
    for i, w in enumerate(want):
        if w != 0xFF:
            assert st[i] == w, (i, index[i], st[i], w)
    # every entry against the single-key calls (n_public = 0 for the key without K points)
    for e, pvk in enumerate([no_k, zero.pvk, two.pvk]):
        pos = [i for i in range(len(index)) if index[i] == e]
        single = pvk.verify_batch(b"".join(proofs[256 * i:256 * i + 256] for i in pos), b"".join(rows[64 * i:64 * i + 32 * npub[e]] for i in pos), n=len(pos), n_public=npub[e])
        assert bytes(st[i] for i in pos) == single, e
    assert pkg.ERR_INPUT_LEN in st and pkg.ERR_NOT_IN_SUBGROUP in st and pkg.ERR_NOT_ON_CURVE in st and pkg.ERR_NOT_MEMBER in st and pkg.ACCEPT in st
    no_k.close()
