"""The synthetic PlonK workload generator (bn254_synth_plonk, _range, _for_inputs: csrc/bn254_capi_dbg.hip) on the CPU.  The generator makes proofs from the KZG
secret of a key it draws itself; whether they are valid is decided HERE, by the oracle's PlonK verifier, for every shape, every proof and every corruption class.
The rest: determinism over threads and ranges, distinctness, lengths, the product's key loader, chosen input rows, and the argument rules."""
import ctypes as C

import pytest

BAD = -1   # BN254_E_BAD_ARG
SHAPES = [(0, 0, 3), (1, 0, 10), (2, 1, 26), (3, 2, 20), (5, 8, 28), (2, 8, 12)]      # (n_public, n_qcp, log2 size)
OPENING, PAIRING, NOT_ON_CURVE, NOT_MEMBER, BSB22 = 7, 8, 3, 2, 9
CLASS_STATUS = [OPENING, PAIRING, NOT_ON_CURVE, NOT_MEMBER, PAIRING, BSB22]


def _rows(inputs, n_public, i):
    return [inputs[32 * (n_public * i + j):32 * (n_public * i + j + 1)] for j in range(n_public)]


def _class(i, e, n_public, n_qcp):
    """the corruption class of proof i (None: valid), with the fall-backs of a key that has no inputs or no commitments"""
    if e <= 0 or i % e != e - 1:
        return None
    c = (i // e) % 6
    if (c == 0 and n_public == 0) or (c in (4, 5) and n_qcp == 0):
        c = 1
    return c


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_oracle_agrees_with_every_expected_status(pkg, O, shape):
    """48 proofs, every second one corrupted: the oracle's status of each equals the generator's, every class the shape has occurs, 24 are accepted"""
    n_public, n_qcp, log2 = shape
    vk, proofs, inputs, exp = pkg.synth_plonk(0x504C0000 + log2, n_public, n_qcp, log2, 48, invalid_every=2, threads=4)
    plen = pkg.lib().bn254_synth_plonk_proof_len(n_qcp)
    assert len(vk) == pkg.lib().bn254_synth_plonk_vk_len(n_qcp) == 34328 + 40 * n_qcp and len(proofs) == 48 * plen and plen == 808 + 96 * n_qcp
    got = bytes(O.plonk_verify(proofs[plen * i:plen * (i + 1)], vk, _rows(inputs, n_public, i)) for i in range(48))
    assert got == exp
    classes = [_class(i, 2, n_public, n_qcp) for i in range(48)]
    assert exp == bytes(pkg.ACCEPT if c is None else CLASS_STATUS[c] for c in classes)
    want = {1, 2, 3} | ({0} if n_public else set()) | ({4, 5} if n_qcp else set())
    assert {c for c in classes if c is not None} == want
    assert exp.count(bytes([pkg.ACCEPT])) >= 24


def test_same_bytes_for_any_thread_count(pkg):
    a = pkg.synth_plonk(11, 3, 2, 20, 40, invalid_every=4, threads=1)
    b = pkg.synth_plonk(11, 3, 2, 20, 40, invalid_every=4, threads=4)
    assert a == b


def test_range_is_a_slice_of_the_full_run(pkg):
    vk, proofs, inputs, exp = pkg.synth_plonk(12, 2, 1, 26, 32, invalid_every=4, threads=2)
    vk2, p2, i2, e2 = pkg.synth_plonk(12, 2, 1, 26, 9, invalid_every=4, threads=3, first=17)
    assert vk2 == vk and p2 == proofs[904 * 17:904 * 26] and i2 == inputs[64 * 17:64 * 26] and e2 == exp[17:26]


def test_seeds_and_shapes_give_different_keys(pkg):
    keys = [pkg.synth_plonk(s, 2, 1, lg, 0)[0] for s, lg in ((1, 26), (2, 26), (1, 25))]
    assert len(set(keys)) == 3
    assert pkg.synth_plonk(1, 2, 1, 26, 0)[0] == keys[0]


def test_proofs_of_a_run_are_pairwise_distinct(pkg):
    for invalid_every in (0, 3):
        vk, proofs, inputs, exp = pkg.synth_plonk(13, 2, 1, 26, 200, invalid_every=invalid_every, threads=4)
        recs = [proofs[904 * i:904 * (i + 1)] for i in range(200)]
        assert len(set(recs)) == 200
        # not only as records: no commitment and no opening proof occurs twice
        for off in (0, 192, 448, 516 + 32 * 7):
            assert len({r[off:off + 64] for r in recs}) == 200
        assert len({inputs[64 * i:64 * (i + 1)] for i in range(200)}) == 200


def test_stride_larger_than_the_proof(pkg):
    vk, proofs, inputs, exp = pkg.synth_plonk(14, 5, 8, 28, 6, invalid_every=3, threads=2)
    vk2, wide, in2, exp2 = pkg.synth_plonk(14, 5, 8, 28, 6, invalid_every=3, threads=2, proof_stride=1664)
    assert (vk2, in2, exp2) == (vk, inputs, exp) and len(wide) == 6 * 1664
    for i in range(6):
        assert wide[1664 * i:1664 * i + 1576] == proofs[1576 * i:1576 * (i + 1)] and wide[1664 * i + 1576:1664 * (i + 1)] == bytes(88)


@pytest.mark.parametrize("shape", [(0, 0, 3), (2, 1, 26), (5, 8, 28)], ids=lambda s: "%d-%d-%d" % s)
def test_key_loads_through_the_product_loader(pkg, shape):
    n_public, n_qcp, log2 = shape
    vk = pkg.synth_plonk(15, n_public, n_qcp, log2, 0)[0]
    pvk = pkg.PreparedPlonkVk(vk)
    assert pvk.n_public == n_public
    pvk.close()


def test_proofs_for_chosen_inputs(pkg, O):
    """rows the caller chose -- zero, r - 1, small values -- are accepted by the oracle, under the key of bn254_synth_plonk for the same arguments"""
    rows = [0, O.R - 1, 1, 2, 0xDEADBEEF, O.R - 2, 1 << 252, 7]
    inputs = b"".join(O.be32(v) for v in rows)
    vk, proofs = pkg.synth_plonk_for_inputs(16, 2, 1, 26, inputs, threads=2)
    assert vk == pkg.synth_plonk(16, 2, 1, 26, 0)[0] and len(proofs) == 4 * 904
    for i in range(4):
        assert O.plonk_verify(proofs[904 * i:904 * (i + 1)], vk, rows[2 * i:2 * i + 2]) == O.ACCEPT
    assert O.plonk_verify(proofs[:904], vk, [0, O.R - 2]) == O.ERR_OPENING_MISMATCH
    # a key without inputs: n proofs from no rows
    vk0, p0 = pkg.synth_plonk_for_inputs(16, 0, 0, 3, b"", n=3)
    assert len({p0[808 * i:808 * (i + 1)] for i in range(3)}) == 3 and all(O.plonk_verify(p0[808 * i:808 * (i + 1)], vk0, []) == O.ACCEPT for i in range(3))


def test_argument_errors_write_nothing(pkg, O):
    L = pkg.lib()
    pkg.synth_plonk(1, 0, 0, 3, 0)      # declares the argument types
    fill = 0xC3

    def call(fn, n_public=2, n_qcp=1, log2=26, n=2, stride=904, null=None, inputs=None):
        vk = (C.c_uint8 * 40000)(*([fill] * 40000)); pr = (C.c_uint8 * 4096)(*([fill] * 4096)); inp = (C.c_uint8 * 4096)(*([fill] * 4096)); ex = (C.c_uint8 * 16)(*([fill] * 16))
        bufs = {"vk": vk, "proofs": pr, "inputs": inp, "expected": ex}
        a = {k: (None if k == null else v) for k, v in bufs.items()}
        if fn == "range":
            rc = L.bn254_synth_plonk_range(1, n_public, n_qcp, log2, 0, n, 2, 1, a["vk"], a["proofs"], stride, a["inputs"], a["expected"])
        elif fn == "plain":
            L.bn254_synth_plonk.argtypes = [C.c_uint64, C.c_size_t, C.c_size_t, C.c_uint, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            rc = L.bn254_synth_plonk(1, n_public, n_qcp, log2, n, 2, 1, a["vk"], a["proofs"], stride, a["inputs"], a["expected"])
        else:
            rows = inputs if inputs is not None else bytes(32 * n_public * n)
            rc = L.bn254_synth_plonk_for_inputs(1, n_public, n_qcp, log2, n, None if null == "inputs" else rows, 1, a["vk"], a["proofs"], stride)
        assert all(bytes(b) == bytes([fill]) * len(b) for b in bufs.values()), "an argument error wrote to a buffer"
        return rc

    for fn in ("range", "plain", "for_inputs"):
        assert call(fn, n_qcp=9, stride=2000) == BAD
        assert call(fn, log2=0) == BAD and call(fn, log2=29) == BAD
        assert call(fn, n_public=6, n_qcp=3, log2=3, stride=1096) == BAD        # 8 rows < 6 + 3
        assert call(fn, n_public=9, n_qcp=0, log2=3, n=1) == BAD
        assert call(fn, stride=903) == BAD
        assert call(fn, null="vk") == BAD and call(fn, null="proofs") == BAD
    assert call("range", null="inputs") == BAD and call("range", null="expected") == BAD and call("for_inputs", null="inputs") == BAD
    assert call("for_inputs", inputs=bytes(96) + O.be32(O.R)) == BAD and call("for_inputs", inputs=b"\xff" * 32 + bytes(96)) == BAD
    assert b"bad argument" in L.bn254_last_error()
    # the limits themselves are accepted: 8 commitments, a domain exactly n_public + n_qcp, n = 0 with no proof buffers
    vk, proofs, inputs, exp = pkg.synth_plonk(1, 0, 8, 3, 2, invalid_every=0)
    assert all(O.plonk_verify(proofs[1576 * i:1576 * (i + 1)], vk, []) == O.ACCEPT for i in range(2))
    vk = (C.c_uint8 * 34368)()
    assert L.bn254_synth_plonk_range(1, 2, 1, 26, 0, 0, 2, 1, vk, None, 904, None, None) == 0 and bytes(vk) == pkg.synth_plonk(1, 2, 1, 26, 0)[0]
