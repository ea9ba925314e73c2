"""The expectations of tests/test_gpu_plonk_stage_values.py proven without a GPU: bn254_dbg_plonk_stages with device -1 -- the host compile of the PlonK stage
source, lambda and the weight derived as the per-key self-test restates them, each sum a plain host sum of the terms the stages wrote -- against
tests/plonk_stage_ref.py, which knows the oracle, hashlib and the ChaCha20 block function and nothing of the stage source.  Every comparison is byte equality."""
import ctypes as C

import pytest

import plonk_stage_ref as ref

SHAPES = [(0, 0, 3), (1, 0, 4), (2, 1, 12), (9, 1, 5), (40, 2, 7), (8, 8, 6)]      # (n_public, n_qcp, log2 rows): those of the GPU tests
N = 24
KEY = [0x9e3779b9, 0x7f4a7c15, 0xf39cc060, 0x5cedc834, 0x1082276b, 0xf3a27251, 0xf86c6a11, 0xd0c18e95, 0x2767f0b1, 0x53d8b4f0, 0x0c4f1a3d]
BAD_ARG = -1


def _seed(shape):
    return 0x57A6E500 + 64 * shape[0] + shape[2]


@pytest.fixture(scope="module")
def batches(pkg):
    """shape -> (prepared key, vk, proofs, inputs, generator's statuses, proof length); made once and never changed"""
    cache = {}

    def get(shape):
        if shape not in cache:
            vk, proofs, inputs, exp = pkg.synth_plonk(_seed(shape), shape[0], shape[1], shape[2], N, invalid_every=3, threads=4)
            cache[shape] = (pkg.PreparedPlonkVk(vk), vk, proofs, inputs, exp, 808 + 96 * shape[1])
        return cache[shape]

    yield get
    for w in cache.values():
        w[0].close()


def test_chacha20_block_rfc8439_and_the_two_streams():
    """RFC 8439 section 2.3.2; lambda and the weight read the block as the issue states it"""
    key, nonce = bytes(range(32)), bytes.fromhex("000000090000004a00000000")
    out = ref.chacha_block(key, 1, nonce)
    assert out == [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
                   0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    import struct
    words = list(struct.unpack("<8I", key)) + list(struct.unpack("<3I", nonce))
    blocks = [ref.chacha_block(key, c, nonce)[:4] for c in range(3, 6)]
    lam1 = int.from_bytes(b"".join(struct.pack("<4I", *b) for b in blocks), "big") % ref.R
    assert ref.lam_of(words, 1) == lam1 and ref.lam_of(words, 0) != lam1
    twisted = struct.pack("<3I", words[8], words[9], words[10] ^ 0x00524c43)
    w = ref.chacha_block(key, 5, twisted)[:4]
    assert ref.weight_of(words, 5) == (w[0] | 1) + (w[1] << 32) + (w[2] << 64) + (w[3] << 96)
    assert ref.weight_of(words, 5) & 1 and ref.weight_of(words, 5) < 1 << 128


def test_hash_to_field_restatement(O, fixtures):
    """hashlib's expand_message_xmd against the oracle's 48 bytes for commitment 0 of the reference's fixture, and against the golden of test_oracle_golden.py"""
    fx, vk = fixtures
    f = fx["fibonacci_plonk"]
    proof = bytes.fromhex(f["raw_proof"])
    got = ref.check_h2f(O, proof, vk, [ref.be32(int(x)) for x in f["public_inputs"]], 1)
    assert got.hex() == "4ed0ec0b9febdbd1a0ddc19e34e284b7146bad6c6e1d7d280158ce06f79a9ad2b2b00696a478f3ea1f47e0f8a9d137fb"
    assert ref.h2f(ref.commitments(proof, 1)[0]) == 0x0F96B0D99F9958D68DBAA54E785873546F6444FD047EE467A6CF86DBDB28BC61
    for msg, n in ((b"", 48), (b"abc", 48), (b"x" * 64, 48), (b"q" * 100, 96)):
        assert O.expand_msg_xmd(msg, b"BSB22-Plonk", n) == ref.expand_message_xmd(msg, b"BSB22-Plonk", n)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_host_compile_of_the_stages_equals_the_oracle(pkg, O, batches, shape):
    """24 proofs, every third invalid: every value of the probe's record, plain and in the weighted form, equals what the oracle gives for that proof under lambda_i
    (and w_i); the digest of the linearised polynomial, which no oracle call gives, is the same curve point in both forms"""
    pvk, vk, proofs, inputs, exp, plen = batches(shape)
    n_public, n_qcp = shape[0], shape[1]
    plain = pkg.dbg_plonk_stages(pvk, proofs, inputs, KEY, n=N, proof_stride=plen, device=-1)
    weighted = pkg.dbg_plonk_stages(pvk, proofs, inputs, KEY, n=N, proof_stride=plen, flags=pkg.FLAG_RLC, device=-1)
    alive = 0
    for i in range(N):
        proof, row = proofs[plen * i:plen * (i + 1)], ref.rows(inputs, n_public, i)
        lam, w = ref.lam_of(KEY, i), ref.weight_of(KEY, i)
        want = ref.expect(O, vk, proof, row, n_qcp, lam, slot=i)
        assert want["oracle_status"] == exp[i]                                   # the generator's statuses are the oracle's
        ref.compare(plain[i], want, "proof %d" % i)
        if want["status1"] == ref.ACCEPT:
            alive += 1
            assert not want.get("ambiguous")
            want_w = dict(want, p0=O.g1_mul(want["p0"], w), p1=O.g1_mul(want["p1"], w))
            ref.compare(weighted[i], want_w, "proof %d, weighted" % i)
            assert weighted[i]["lin"] == plain[i]["lin"]
            # the free identity, stated on its own: the opening the stage computed is the first claimed value exactly where the oracle saw no mismatch
            assert plain[i]["lin_opening"] == proof[516:548]
        else:
            ref.compare(weighted[i], want, "proof %d, weighted" % i)
            assert plain[i]["lin_opening"] != proof[516:548]
    assert alive >= 14 and {e for e in exp} >= {1, 8}
    # values of proof i do not depend on n, nor on what lies behind the proof in its record
    wide = b"".join(proofs[plen * i:plen * (i + 1)] + b"\xa5" * 13 for i in range(5))
    assert pkg.dbg_plonk_stages(pvk, wide, inputs, KEY, n=5, proof_stride=plen + 13, device=-1) == plain[:5]


def test_lambda_stream_on_the_host_compile(pkg, batches):
    """one nonce bit moves every lambda; the lambdas of a batch are pairwise distinct; the weights are odd, distinct, and not the lambda stream"""
    pvk, vk, proofs, inputs, exp, plen = batches((2, 1, 12))
    other = list(KEY); other[9] ^= 1 << 17
    a = pkg.dbg_plonk_stages(pvk, proofs, inputs, KEY, n=N, proof_stride=plen, device=-1)
    b = pkg.dbg_plonk_stages(pvk, proofs, inputs, other, n=N, proof_stride=plen, device=-1)
    live = [i for i in range(N) if a[i]["status1"] == ref.ACCEPT]
    assert len(live) >= 14 and all(a[i]["lambda"] != b[i]["lambda"] for i in live)
    assert len({a[i]["lambda"] for i in live}) == len(live)
    assert all(a[i]["lambda"] == ref.be32(ref.lam_of(KEY, i)) and b[i]["lambda"] == ref.be32(ref.lam_of(other, i)) for i in live)
    ws = [ref.weight_of(KEY, i) for i in range(N)]
    assert all(w & 1 for w in ws) and len(set(ws)) == N and not {w for w in ws} & {ref.lam_of(KEY, i) % (1 << 128) for i in range(3 * N)}


def test_argument_errors(pkg, batches):
    """every argument error is BN254_E_BAD_ARG, before a device is looked at (this machine has none: any other code would be the device's)"""
    pvk, vk, proofs, inputs, exp, plen = batches((2, 1, 12))
    L = pkg.lib()
    fn = L.bn254_dbg_plonk_stages
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint, C.c_void_p, C.c_int]
    out = (C.c_uint8 * (560 * 4097))()
    key = (C.c_uint32 * 11)(*KEY)
    good = (pvk._h, proofs, plen, inputs, 2, 4, key, 0, out, 0)

    def call(**kw):
        names = ("pvk", "proofs", "stride", "inputs", "n_public", "n", "key", "flags", "out", "device")
        return fn(*[kw.get(k, v) for k, v in zip(names, good)])

    for bad in (dict(pvk=None), dict(proofs=None), dict(inputs=None), dict(key=None), dict(out=None), dict(n=0), dict(n=4097), dict(flags=1), dict(flags=0x80), dict(device=-2)):
        assert call(**bad) == BAD_ARG, bad
    assert call(device=-1) == 0
    fk = L.bn254_dbg_plonk_stages_keys
    fk.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint, C.c_void_p, C.c_int]
    arr = (C.c_void_p * 1)(pvk._h.value)
    idx = (C.c_uint32 * 4)(0, 0, 0, 0)
    goodk = (arr, 1, idx, proofs, plen, inputs, 64, 4, key, 0, out, 0)

    def callk(**kw):
        names = ("pvks", "n_keys", "idx", "proofs", "stride", "inputs", "in_stride", "n", "key", "flags", "out", "device")
        return fk(*[kw.get(k, v) for k, v in zip(names, goodk)])

    bad_idx = (C.c_uint32 * 4)(0, 1, 0, 0)
    for bad in (dict(pvks=None), dict(n_keys=0), dict(idx=None), dict(proofs=None), dict(inputs=None), dict(key=None), dict(out=None), dict(n=0), dict(n=4097), dict(flags=1),
                dict(device=-1), dict(stride=903), dict(in_stride=32), dict(idx=bad_idx)):
        assert callk(**bad) == BAD_ARG, bad
