"""BN254_FLAG_COMPRESSED_PROOFS on the CPU: the host compile of k_g16_decompress's body (bn254_dbg_g16_decompress, csrc/bn254_codec.h) against the C ABI's
own codecs (bn254_g1_decompress / bn254_g2_decompress, unchecked, gnark root order) component by component, and against the oracle on valid points; and the
argument checks of the batch entries for the new flag (refused before any device is touched)."""
import ctypes as C
import random

import pytest

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
ONES = b"\xff" * 256


def _dec1(L, b):
    st = C.c_uint8(0xEE); o = (C.c_uint8 * 64)()
    assert L.bn254_g1_decompress(bytes(b), o, 0, C.byref(st)) == 0
    return st.value, bytes(o)


def _dec2(L, b, mode=1):
    st = C.c_uint8(0xEE); o = (C.c_uint8 * 128)()
    assert L.bn254_g2_decompress(bytes(b), o, mode, 0, C.byref(st)) == 0
    return st.value, bytes(o)


def _expected(pkg, rec):
    """The definition: the three unchecked decompressions (G2 in gnark's order); any failure -> (1, all ones)."""
    L = pkg.lib()
    sa, a = _dec1(L, rec[0:32]); sb, b = _dec2(L, rec[32:96]); sc, c = _dec1(L, rec[96:128])
    ok = sa == pkg.ACCEPT and sb == pkg.ACCEPT and sc == pkg.ACCEPT
    return (0, a + b + c) if ok else (1, ONES)


def _check_records(pkg, recs, stride=128):
    buf = b"".join(r + bytes(stride - 128) for r in recs)
    raw, pre = pkg.dbg_g16_decompress(buf, len(recs), stride)
    bad = 0
    for i, r in enumerate(recs):
        e_pre, e_raw = _expected(pkg, r)
        assert pre[i] == e_pre, (i, r.hex())
        assert raw[256 * i:256 * (i + 1)] == e_raw, (i, r.hex())
        bad += e_pre
    return bad


def _x_bytes(x, flag):
    b = bytearray(x.to_bytes(32, "big"))
    b[0] = (b[0] & 0x3f) | (flag << 6)
    return bytes(b)


@pytest.fixture(scope="module")
def proofs(pkg):
    n = 1200
    vk, proofs, inputs, expected = pkg.synth_groth16(0xC0DEC0DE, 2, n, invalid_every=0, agree=True, threads=8)
    return [proofs[256 * i:256 * (i + 1)] for i in range(n)]


def test_probe_matches_host_codecs_on_valid_proofs(pkg, O, proofs):
    """Thousands of valid points (1200 proofs: 2400 G1, 1200 G2): the probe gives back the raw proof, byte for byte, and agrees with the oracle's codecs."""
    recs = [pkg.compress_proof(p) for p in proofs]
    raw, pre = pkg.dbg_g16_decompress(b"".join(recs))
    assert pre == bytes(len(recs))
    assert raw == b"".join(proofs)
    for i in range(0, len(recs), 97):   # a sample through the oracle's own decoders (gnark order)
        r = recs[i]
        s1, a = O.decompress_g1(r[0:32]); s2, b = O.decompress_g2(r[32:96], O.MODE_GNARK); s3, c = O.decompress_g1(r[96:128])
        assert (s1, s2, s3) == (O.ACCEPT,) * 3 and a + b + c == proofs[i]


def test_probe_edge_records(pkg, proofs):
    """x >= p, non-residue x for G1 and G2, all four flag values, infinity with and without trailing bytes, x.c1 = 0, and G2 points whose c0 and lexicographic
    root orders disagree: statuses and bytes as the C ABI's codecs give them, per component."""
    L = pkg.lib()
    rng = random.Random(0xC0)
    base = [pkg.compress_proof(p) for p in proofs[:64]]
    recs = []
    for k, r in enumerate(base):
        a, b, c = r[0:32], r[32:96], r[96:128]
        xa = int.from_bytes(a, "big") & ((1 << 254) - 1)
        xc1 = int.from_bytes(b[0:32], "big") & ((1 << 254) - 1)
        fa, fb = a[0] >> 6, b[0] >> 6
        # x >= p (silently reduced): x + p where it still fits under the flag bits
        if xa + P < (1 << 254):
            recs.append(_x_bytes(xa + P, fa) + b + c)
        if xc1 + P < (1 << 254):
            recs.append(a + _x_bytes(xc1 + P, fb) + b[32:] + c)
        x0 = int.from_bytes(b[32:64], "big")
        if x0 + P < (1 << 256):
            recs.append(a + b[0:32] + (x0 + P).to_bytes(32, "big") + c)
        # every flag value on each point
        for f in range(4):
            recs.append(_x_bytes(xa, f) + b + c)
            recs.append(a + _x_bytes(xc1, f) + b[32:] + c)
            recs.append(a + b + _x_bytes(int.from_bytes(c, "big") & ((1 << 254) - 1), f))
        # random x: about half of them are non-residues, for G1 and for G2
        for f in (2, 3):
            recs.append(_x_bytes(rng.randrange(P), f) + b + c)
            recs.append(a + _x_bytes(rng.randrange(P), f) + rng.randrange(P).to_bytes(32, "big") + c)
            recs.append(a + b + _x_bytes(rng.randrange(P), f))
        # x.c1 = 0
        for f in (2, 3):
            recs.append(a + _x_bytes(0, f) + rng.randrange(P).to_bytes(32, "big") + c)
        if k < 4:
            z32 = bytes(32)
            recs.append(bytes([0x40]) + z32[1:] + b + c)                        # G1 infinity: MALFORMED (3 is a non-residue)
            recs.append(a + bytes([0x40]) + z32[1:] + z32 + c)                  # G2 infinity: the generator
            recs.append(a + bytes([0x40]) + z32[1:] + b[32:] + c)               # G2 infinity, x.c0 bytes not looked at
            recs.append(a + bytes([0x40]) + z32[1:30] + b"\x01\x00" + z32 + c)  # G2 infinity with a trailing bit: MALFORMED
            recs.append(a + bytes([0x41]) + z32[1:] + z32 + c)                  # ... in the flag byte: MALFORMED
            recs.append(a + b + bytes([0x40]) + z32[30:31] + b"\x07" + z32[:29])  # G1 infinity with trailing bytes: MALFORMED
    bad = _check_records(pkg, recs)
    assert 0 < bad < len(recs)
    # G2 points whose two readings of the root order disagree: the probe follows gnark's (mode 1) on them
    disagree = 0
    for r in recs:
        s1, y1 = _dec2(L, r[32:96], 1); s0, y0 = _dec2(L, r[32:96], 0)
        if s1 == pkg.ACCEPT and s0 == pkg.ACCEPT and y0 != y1:
            disagree += 1
    assert disagree > 10


def test_probe_strides(pkg, proofs):
    """The probe reads records at any stride >= 128 and ignores the bytes past 128."""
    recs = [pkg.compress_proof(p) for p in proofs[:16]]
    want, _ = pkg.dbg_g16_decompress(b"".join(recs))
    for stride in (131, 324):
        buf = b"".join(r + bytes([0xA5]) * (stride - 128) for r in recs)
        raw, pre = pkg.dbg_g16_decompress(buf, len(recs), stride)
        assert pre == bytes(len(recs)) and raw == want
    with pytest.raises(pkg.Bn254Error):
        pkg.dbg_g16_decompress(b"".join(recs), len(recs), 127)


def test_batch_arguments_of_the_new_flag(pkg):
    """Refused by check_batch_args before any device is touched: stride 128 without the flag, stride 127 with it, flag 8, and flag 4 on the PlonK entries.
    The flag itself with stride 128 passes the check (n = 0: nothing to do)."""
    L = pkg.lib()
    vk, proofs, inputs, _ = pkg.synth_groth16(7, 2, 1, invalid_every=0, agree=True)
    h = C.c_void_p()
    assert L.bn254_groth16_vk_prepare(vk, len(vk), 1, C.byref(h)) == 0
    try:
        st = (C.c_uint8 * 4)()
        rec = pkg.compress_proof(proofs[:256]) * 4
        BAD = -1
        assert L.bn254_groth16_verify_batch(h, rec, 128, inputs * 4, 2, 4, st, 0, 0) == BAD
        assert L.bn254_groth16_verify_batch(h, rec, 127, inputs * 4, 2, 4, st, 0, 4) == BAD
        assert L.bn254_groth16_verify_batch(h, proofs * 4, 256, inputs * 4, 2, 4, st, 0, 8) == BAD
        assert L.bn254_groth16_verify_batch(h, proofs * 4, 256, inputs * 4, 2, 4, st, 0, 4 | 8) == BAD
        assert L.bn254_groth16_verify_batch_multi(h, rec, 128, inputs * 4, 2, 4, st, C.c_uint64(1), 0) == BAD
        assert L.bn254_groth16_verify_batch_multi(h, rec, 127, inputs * 4, 2, 4, st, C.c_uint64(1), 4) == BAD
        assert L.bn254_groth16_verify_batch_device(h, rec, 128, inputs * 4, 2, 4, st, 0, None, 0) == BAD
        assert L.bn254_groth16_verify_batch_device(h, rec, 120, inputs * 4, 2, 4, st, 0, None, 4) == BAD
        assert L.bn254_groth16_verify_batch(h, rec, 128, inputs * 4, 2, 0, st, 0, 4) == 0
        assert L.bn254_groth16_verify_batch(h, rec, 128, inputs * 4, 2, 0, st, 0, 4 | 1 | 2) == 0
    finally:
        L.bn254_groth16_vk_free(h)
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pvk_bytes = open(os.path.join(root, "tests", "golden", "plonk_vk.bin"), "rb").read()
    ph = C.c_void_p()
    assert L.bn254_plonk_vk_prepare(pvk_bytes, len(pvk_bytes), C.byref(ph)) == 0
    try:
        st = (C.c_uint8 * 1)()
        proof = bytes(904)
        assert L.bn254_plonk_verify_batch_flags(ph, proof, 904, bytes(64), 2, 1, st, 0, 4) == -1
        assert L.bn254_plonk_verify_batch_multi(ph, proof, 904, bytes(64), 2, 1, st, C.c_uint64(1), 4) == -1
        assert L.bn254_plonk_verify_batch_device(ph, proof, 904, bytes(64), 2, 1, st, 0, None, 4) == -1
    finally:
        L.bn254_plonk_vk_free(ph)
