"""The DIRECT form of a Groth16 batch over many keys (include/bn254_verify.h, "Batches over many keys": small batches; k_coop12_miller_g16_keys, twelve lanes per
proof, the key read per proof) on the GPU.

The definition of correctness is that of tests/test_gpu_multikey.py: status[i] is what the single-key entry writes for (proof i, its key).  Every case compares the
mixed batch with the generator's expected statuses (where the records are the generator's), with per-key bn254_groth16_verify_batch calls on the same GPU and,
EVERY proof, with the CPU oracle O.groth16_verify_many (_full_check).  The oracle knows neither flag: under BN254_FLAG_STRICT_SCALARS its byte is replaced by
NOT_MEMBER where one of the key's inputs is >= r, for compressed records it runs on the raw record the compressed one was made from and its byte is replaced by
MALFORMED where the test broke the record -- both by the header's definition, not by what the library answers.  The shapes are the boundaries of ONE wavefront (five
proofs, lanes 60..63 shadowing the fifth), not of a batch.  No case looks into the code object; no case is meant to fault."""
import pytest

from test_gpu_multikey import Key, Mixed, NO_K, R

pytestmark = pytest.mark.gpu

PER_WAVE = 5                # csrc/bn254_coop12.hip: C12_PER_WAVE
WIDTHS = (0, 1, 2, 5, 16)    # n_public of the keys of `keys`, per mode


@pytest.fixture(scope="module")
def keys(pkg):
    """n_public 0, 1, 2, 5, 16 in both modes (keys 0..4 reference, 5..9 gnark), 24 proofs each, every 4th invalid (classes REJECT, REJECT, NOT_MEMBER,
    NOT_IN_SUBGROUP, NOT_ON_CURVE in turn)"""
    out = [Key(pkg, 0x4D0000 + 16 * m + p, p, 24, mode=m, invalid_every=4, threads=8) for m in (pkg.VK_REFERENCE, pkg.VK_GNARK) for p in WIDTHS]
    yield out
    for k in out:
        k.pvk.close()


@pytest.fixture(scope="module")
def no_k(pkg, keys):
    """the zero-input key's bytes without K points: every proof that loads answers INPUT_LEN"""
    vk = keys[0].vk[:288] + (0).to_bytes(4, "big") + keys[0].vk[292 + 32:]
    pvk = pkg.PreparedVk(vk)
    assert pvk.n_public == NO_K
    yield vk, pvk
    pvk.close()


@pytest.fixture(autouse=True)
def restore_knob(pkg):
    yield
    pkg.set_keys_params(_DEFAULT[0])


_DEFAULT = []


@pytest.fixture(scope="module", autouse=True)
def find_default(pkg):
    """the hand-over the library starts with: the largest n the plan probe sends to the direct form (the knob has no getter)"""
    lo, hi = 0, 30721
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pkg.dbg_keys_plan(mid, 1)[0] == 1 else (lo, mid)
    assert lo >= 1, "the direct form is switched off in this process (BN254_KEYS_COOP_MAX=0 or BN254_COOP=0): nothing here would test it"
    _DEFAULT[:] = [lo]
    yield
    pkg.set_keys_params(lo)


class Ent:
    """an entry of a key list: what the single-key call and the oracle need"""

    def __init__(self, vk, pvk, n_public, mode=0):
        self.vk, self.pvk, self.n_public, self.mode = vk, pvk, n_public, mode


def _ents(mx):
    return [Ent(mx.keys[k].vk, mx.keys[k].pvk, mx.keys[k].n_public, mx.keys[k].mode) for k in mx.key_list]


def _oracle(O, ents, index, raw, rows, stride):
    """O.groth16_verify_many for every proof of the batch under the list entry its index names, one call per entry, in batch order"""
    out = bytearray(len(index))
    for e, ent in enumerate(ents):
        pos = [i for i in range(len(index)) if index[i] == e]
        if not pos:
            continue
        st = O.groth16_verify_many(b"".join(raw[256 * i:256 * i + 256] for i in pos), 256, ent.vk, b"".join(rows[stride * i:stride * i + 32 * ent.n_public] for i in pos),
                                   ent.n_public, len(pos), O.MODE_GNARK if ent.mode else O.MODE_REFERENCE)
        for i, b in zip(pos, st):
            out[i] = b
    return bytes(out)


def _full_check(pkg, O, ks, ents, index, raw, rows, stride, exp=None, want_form=1, flags=0, comp=None, broken=(), oracle=None):
    """One batch through the host entry against the generator (exp), per-key single-key calls on the same GPU with the same flags, and the oracle for EVERY proof.
    raw: the 256-byte records; comp: their compressed form when that is what is submitted (broken: positions whose record the test made undecodable).
    oracle: bytes of an earlier _oracle call on the same batch (computed once, shared).  Returns (statuses, oracle bytes)."""
    n = len(index)
    rec, sub = (128, bytes(comp)) if comp is not None else (256, bytes(raw))
    st = ks.verify_batch(index, sub, bytes(rows), input_stride=stride, flags=flags, compressed=comp is not None)
    assert len(st) == n and ks.last_form() == want_form
    if exp is not None:
        bad = [i for i in range(n) if st[i] != exp[i]]
        assert st == exp, ("generator", len(bad), [(i, index[i], st[i], exp[i]) for i in bad[:10]])
    for e, ent in enumerate(ents):
        pos = [i for i in range(n) if index[i] == e]
        if pos:
            single = ent.pvk.verify_batch(b"".join(sub[rec * i:rec * i + rec] for i in pos), b"".join(rows[stride * i:stride * i + 32 * ent.n_public] for i in pos), n=len(pos),
                                          n_public=ent.n_public, flags=flags & ~pkg.FLAG_RLC, compressed=comp is not None)
            assert bytes(st[i] for i in pos) == single, ("single-key calls", e)
    if oracle is None:
        oracle = _oracle(O, ents, index, raw, rows, stride)
    want = bytearray(oracle)
    if flags & pkg.FLAG_STRICT_SCALARS:
        for i in range(n):
            if any(int.from_bytes(rows[stride * i + 32 * s:stride * i + 32 * s + 32], "big") >= R for s in range(ents[index[i]].n_public)):
                want[i] = pkg.ERR_NOT_MEMBER
    for i in broken:
        want[i] = pkg.ERR_MALFORMED
    bad = [i for i in range(n) if st[i] != want[i]]
    assert st == bytes(want), ("oracle", len(bad), [(i, index[i], st[i], want[i]) for i in bad[:10]])
    return st, oracle


def _check(pkg, O, mx, ks, want_form=1, **kw):
    if not hasattr(mx, "oracle_bytes"):
        mx.oracle_bytes = None
    st, mx.oracle_bytes = _full_check(pkg, O, ks, _ents(mx), mx.index, mx.proofs, mx.rows, mx.stride, exp=mx.exp, want_form=want_form, oracle=mx.oracle_bytes, **kw)
    return st


@pytest.mark.parametrize("n", [1, 4, 5, 6, 11])
def test_one_wavefront(pkg, O, keys, n):
    """the five groups of a wavefront hold five keys of five widths; at n = 5 the 16-input key sits in group 4, the one lanes 60..63 shadow; n = 6 and 11 leave a
    wavefront with one live group; invalid proofs of every class among them"""
    order = [1, 7, 3, 5, 4, 9, 2, 0, 8, 6]                    # keys by position: widths 1, 2, 5, 0, 16 | 16, 2, 0, 5, 1
    pick = {1: [0], 4: [3, 0, 7, 11], 5: [0, 3, 7, 1, 2], 6: [0, 11, 15, 19, 3, 1], 11: [3, 7, 11, 15, 19, 23, 0, 1, 2, 4, 5]}[n]
    entries = [(order[i % 10], pick[i]) for i in range(n)]
    if n == 5:
        assert keys[entries[4][0]].n_public == 16
    mx = Mixed(keys, entries=entries)
    assert len({k for k, _ in entries}) == min(n, 10)
    st = _check(pkg, O, mx, mx.key_set(pkg))
    assert pkg.ACCEPT in st and (n == 1 or any(s != pkg.ACCEPT for s in st))


def test_the_index_is_honoured_inside_a_wavefront(pkg, O):
    """valid proofs of key a and key b (same width) ALTERNATE, so every wavefront holds both; the same records under the other key are what the oracle says for
    (proof, other key), never ACCEPT: a kernel that took one key per wavefront passes every sorted batch and fails here"""
    a, b = Key(pkg, 0x4D1001, 2, 8, invalid_every=0, threads=4), Key(pkg, 0x4D1002, 2, 8, invalid_every=0, threads=4)
    mx = Mixed([a, b], entries=[(i & 1, i >> 1) for i in range(16)])
    ks = pkg.KeySet([a.pvk, b.pvk])
    n = 16
    crossed = [1 - k for k in mx.index]
    st, _ = _full_check(pkg, O, ks, _ents(mx), mx.index + crossed, mx.proofs + mx.proofs, mx.rows + mx.rows, mx.stride)
    assert st[:n] == mx.exp == bytes([pkg.ACCEPT]) * n
    assert pkg.ACCEPT not in st[n:]
    a.pvk.close(); b.pvk.close()


@pytest.fixture(scope="module")
def twelve_small(pkg):
    """twelve keys, n_public 0, 1, 2, 5, 8, 16 in both modes, 50 proofs each, every 7th invalid: all five classes per key"""
    out = [Key(pkg, 0x4D2000 + 16 * m + p, p, 50, mode=m, invalid_every=7, threads=8) for m in (pkg.VK_REFERENCE, pkg.VK_GNARK) for p in (0, 1, 2, 5, 8, 16)]
    yield out
    for k in out:
        k.pvk.close()


def test_both_forms_one_process(pkg, O, twelve_small):
    """600 proofs over twelve keys in the grouped and in the direct form: the same bytes, every one the oracle's (computed once for both runs)"""
    mx = Mixed(twelve_small, seed=21)
    assert len(mx.entries) == 600
    ks = mx.key_set(pkg)
    pkg.set_keys_params(0)
    grouped = _check(pkg, O, mx, ks, want_form=0)
    pkg.set_keys_params(_DEFAULT[0])
    direct = _check(pkg, O, mx, ks, want_form=1)
    assert set(direct) == {0, 1, 2, 3, 4}
    assert grouped == direct == mx.exp


def test_hand_over(pkg, O, twelve_small):
    pkg.set_keys_params(64)
    mx = Mixed(twelve_small, seed=22)
    ks = mx.key_set(pkg)
    for n, form in ((64, 1), (65, 0)):
        sub = Mixed(twelve_small, entries=mx.entries[:n])
        assert pkg.dbg_keys_plan(n, 12)[0] == form
        _check(pkg, O, sub, ks, want_form=form)


def test_l_is_the_identity(pkg, O):
    """keys whose generator makes L = K0 + sum x_i K_i the identity for the proofs with index = 3 (mod 7): the line at L has the value 1 and the proofs stay ACCEPT
    (L projective in this kernel: Z_L = 0)"""
    ks_ = [Key.__new__(Key) for _ in range(3)]
    for key, p in zip(ks_, (1, 2, 16)):
        key.vk, key.proofs, key.inputs, key.exp = pkg.synth_groth16(0x4D3000 + p, p, 14, invalid_every=5, agree=True, threads=4, l_identity=True)
        key.n_public, key.n, key.mode = p, 14, 0
        key.pvk = pkg.PreparedVk(key.vk)
        assert all(key.exp[j] == pkg.ACCEPT for j in range(14) if j % 7 == 3)
    mx = Mixed(ks_, entries=[(i % 3, i // 3) for i in range(42)])
    st = _check(pkg, O, mx, mx.key_set(pkg))
    assert all(st[i] == pkg.ACCEPT for i, (_, j) in enumerate(mx.entries) if j % 7 == 3)
    for key in ks_:
        key.pvk.close()


def _mutations(pkg, two):
    """a valid record of the two-input key and the mutations of test_edge_keys_in_a_set: C.x >= p, C off the curve, A off the curve, B outside G2, both"""
    j0 = next(j for j in range(two.n) if two.exp[j] == pkg.ACCEPT)
    b_outside = next(two.proof(j) for j in range(two.n) if two.exp[j] == pkg.ERR_NOT_IN_SUBGROUP)
    good = two.proof(j0)
    big = bytearray(good); big[192:224] = b"\xff" * 32                     # C.x >= p
    offc = bytearray(good); offc[255] ^= 1                                 # C off the curve
    offa = bytearray(good); offa[63] ^= 1                                  # A off the curve
    both = bytearray(b_outside); both[255] ^= 1                            # B outside G2 and C off the curve: B's error comes first
    return j0, [good, bytes(big), bytes(offc), bytes(offa), b_outside, bytes(both)]


def test_loader_errors_and_precedence(pkg, O, keys, no_k):
    """the record mutations of test_edge_keys_in_a_set under the key without K points, the zero-input key and a two-input key, adjacent in one wavefront; first a
    wavefront whose five proofs all fail to load, then live ones"""
    no_k_vk, no_k_pvk = no_k
    zero, two = keys[0], keys[2]
    ks = pkg.KeySet([no_k_pvk, zero.pvk, two.pvk])
    ents = [Ent(no_k_vk, no_k_pvk, 0), Ent(zero.vk, zero.pvk, 0), Ent(two.vk, two.pvk, 2)]
    j0, recs = _mutations(pkg, two)
    # wavefront 0: five records whose A does not load (no pending proof), under all three keys
    plan = [(3, e % 3) for e in range(PER_WAVE)] + [(r, e) for r in range(6) for e in range(3)]
    index = [e for _, e in plan]
    st, _ = _full_check(pkg, O, ks, ents, index, b"".join(recs[r] for r, _ in plan), two.row(j0) * len(plan), 64)
    assert {pkg.ERR_INPUT_LEN, pkg.ERR_NOT_IN_SUBGROUP, pkg.ERR_NOT_ON_CURVE, pkg.ERR_NOT_MEMBER, pkg.ACCEPT} <= set(st)
    assert st[:PER_WAVE] == bytes([pkg.ERR_NOT_ON_CURVE]) * PER_WAVE


def _five_widths(pkg, keys, n):
    """n valid proofs, five per wavefront under keys of widths 1, 2, 16, 5, 0"""
    order = [1, 2, 4, 3, 0]
    valid = {k: [j for j in range(keys[k].n) if keys[k].exp[j] == pkg.ACCEPT] for k in order}
    return Mixed(keys, entries=[(order[i % 5], valid[order[i % 5]][i // 5]) for i in range(n)])


def test_flags(pkg, O, keys):
    mx = _five_widths(pkg, keys, 20)
    ks = mx.key_set(pkg)
    assert _check(pkg, O, mx, ks, flags=pkg.FLAG_RLC) == bytes([pkg.ACCEPT]) * 20      # accepted and ignored
    # strict scalars: x + r in the LAST input of the 16-input key's proof (its neighbours are narrower: a kernel that took a neighbour's width misses it) and in the
    # only input of a 1-input key; the bytes behind a narrower key's inputs in its row hold a value >= r already (0xa5...), which must NOT count
    rows = bytearray(mx.rows)
    hit = []
    for i, (k, j) in enumerate(mx.entries):
        p = keys[k].n_public
        if p in (16, 1) and i % 2 == 0:
            off = mx.stride * i + 32 * (p - 1)
            x = int.from_bytes(rows[off:off + 32], "big")
            assert x + R < 1 << 256
            rows[off:off + 32] = (x + R).to_bytes(32, "big"); hit.append(i)
    assert len(hit) >= 3
    ents = _ents(mx)
    # (the oracle reduces an input mod r, so its bytes for the changed rows are those of the unchanged ones: computed once)
    st, _ = _full_check(pkg, O, ks, ents, mx.index, mx.proofs, rows, mx.stride, flags=pkg.FLAG_STRICT_SCALARS)
    assert [i for i in range(20) if st[i] == pkg.ERR_NOT_MEMBER] == hit and st.count(bytes([pkg.ACCEPT])) == 20 - len(hit)
    _full_check(pkg, O, ks, ents, mx.index, mx.proofs, rows, mx.stride, exp=mx.exp)      # the default policy: x + r is x
    # compressed records; one that does not decompress is MALFORMED
    comp = bytearray(b"".join(pkg.compress_proof(mx.proofs[256 * i:256 * i + 256]) for i in range(20)))
    comp[128 * 7] &= 0x3f                                                        # compression flag 00 on A
    st, _ = _full_check(pkg, O, ks, ents, mx.index, mx.proofs, mx.rows, mx.stride, comp=comp, broken=[7], oracle=mx.oracle_bytes)
    assert st[7] == pkg.ERR_MALFORMED and st.count(bytes([pkg.ACCEPT])) == 19


def test_device_entry(pkg, O, keys):
    """indices outside the list at positions 0, 3 and n - 1: one on a record with a loader error, one in a wavefront none of whose proofs is pending; those proofs
    are MALFORMED, the others what the host entry, the single-key calls and the oracle say, the bytes behind d_status untouched; the host entry refuses the vector
    with BN254_E_BAD_ARG"""
    import torch
    n = 13
    mx = _five_widths(pkg, keys, n)
    _, recs = _mutations(pkg, keys[2])
    offa = recs[3]
    proofs = bytearray(mx.proofs)
    proofs[256 * 3:256 * 4] = offa                       # position 3: a loader error AND (below) an index outside the list
    for i in range(10, 13):                              # the last wavefront (proofs 10..12): nothing loads
        proofs[256 * i:256 * i + 256] = offa
    ks = mx.key_set(pkg)
    host, _ = _full_check(pkg, O, ks, _ents(mx), mx.index, proofs, mx.rows, mx.stride)
    assert host[3] == pkg.ERR_NOT_ON_CURVE and host[10:] == bytes([pkg.ERR_NOT_ON_CURVE]) * 3 and host.count(bytes([pkg.ACCEPT])) == 9
    dev = torch.device("cuda:0")
    ks.reserve(n)
    d_p = torch.frombuffer(proofs, dtype=torch.uint8).to(dev); d_r = torch.frombuffer(bytearray(mx.rows), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(dev)
    for bad in ([], [0, 3, n - 1]):
        index = list(mx.index)
        for i in bad:
            index[i] = len(keys) + i
        d_i = torch.tensor(index, dtype=torch.int64).to(torch.int32).to(dev)
        d_s = torch.full((n + 8,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ks.verify_batch_device(d_i.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), n, input_stride=mx.stride, stream=stream.cuda_stream)
        stream.synchronize()
        got = bytes(d_s.cpu().numpy().tobytes())
        want = bytearray(host)
        for i in bad:
            want[i] = pkg.ERR_MALFORMED
        assert got[:n] == bytes(want), bad
        assert got[n:] == b"\xee" * 8
        assert ks.last_form() == 1
        if bad:
            with pytest.raises(pkg.Bn254Error, match=r"bn254 error -1: .*key_index\[0\] = 10 is outside the list of 10 keys"):      # BN254_E_BAD_ARG: the host entry checks the whole vector first
                mx.run(ks, index, proofs=bytes(proofs))
