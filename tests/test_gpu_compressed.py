"""GPU tests of BN254_FLAG_COMPRESSED_PROOFS (k_g16_decompress, then the raw pipeline, then k_g16_status_merge): every status byte equals the definition of
include/bn254_verify.h -- the raw batch of the host-decompressed records on the GPU, MALFORMED where a record does not decompress -- through the host, device
and multi entries, the cooperative and the lane ranges, a batch of two workspace chunks, BN254_FLAG_RLC (narrow and wide keys, malformed records inside
groups), BN254_FLAG_STRICT_SCALARS, strides 128 / 131 / 324 and a BN254_VK_REFERENCE key; a sample against the oracle."""
import random

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return pkg.lib()


def _g2_non_residue(pkg, seed):
    """A compressed G2 coordinate (flag 0b10) whose x^3 + b' has no square root."""
    import ctypes as C
    rng = random.Random(seed)
    L = pkg.lib()
    st = C.c_uint8(); o = (C.c_uint8 * 128)()
    while True:
        b = bytearray(rng.randrange(1 << 254).to_bytes(32, "big") + rng.randrange(1 << 255).to_bytes(32, "big")); b[0] = (b[0] & 0x3f) | 0x80
        L.bn254_g2_decompress(bytes(b), o, 1, 0, C.byref(st))
        if st.value == pkg.ERR_MALFORMED:
            return bytes(b)


def _compress_batch(pkg, proofs, n, seed, bad_every=11, invalid_every=0):
    """Compress the raw proofs; every bad_every-th record (and every record the codec cannot compress: A off the curve, A.x >= p) is replaced by a record that
    does not decompress (or decompresses to the G2 generator).  Returns (records, raw records the definition gives, pre bytes: 1 = MALFORMED).  The generator's
    invalid proofs (index = invalid_every - 1 mod invalid_every) may carry points off the curve, which compress to a different point: their definition is
    taken from the codec like that of the replaced records."""
    rng = random.Random(seed)
    nonres, z = _g2_non_residue(pkg, seed), bytes(32)
    recs, special = [], {}
    for i in range(n):
        raw = proofs[256 * i:256 * (i + 1)]
        try:
            c = pkg.compress_proof(raw)
        except pkg.Bn254Error:
            c = None
        if c is None or i % bad_every == bad_every - 1:
            base = c or bytes([0x80]) + bytes(127)
            kind = rng.randrange(5)
            if kind == 0:
                c = bytes([base[0] & 0x3f]) + base[1:]                       # flag 0b00 on A
            elif kind == 1:
                c = base[:96] + bytes([0x40]) + z[1:]                           # G1 infinity on C
            elif kind == 2:
                c = base[:32] + nonres + base[96:]                              # B: x^3 + b' has no root
            elif kind == 3:
                c = base[:32] + bytes([0x40]) + z[1:31] + b"\x01" + z + base[96:]  # G2 infinity with a trailing bit
            else:
                c = base[:32] + bytes([0x40]) + z[1:] + z + base[96:]           # G2 infinity: decompresses (to the generator)
            special[i] = c
        elif invalid_every and i % invalid_every == invalid_every - 1:
            special[i] = c
        recs.append(c)
    # the definition on the special records (host compile of the codec; tests/test_compressed_cpu.py pins it to bn254_g{1,2}_decompress); every other record
    # was compressed from a valid proof's points and decompresses to them exactly
    idx = sorted(special)
    sraw, spre = pkg.dbg_g16_decompress(b"".join(special[i] for i in idx), len(idx)) if idx else (b"", b"")
    raw_out, pre = bytearray(proofs[:256 * n]), bytearray(n)
    for k, i in enumerate(idx):
        pre[i] = spre[k]
        raw_out[256 * i:256 * (i + 1)] = sraw[256 * k:256 * (k + 1)] if not spre[k] else proofs[256 * i:256 * (i + 1)]
    return b"".join(recs), bytes(raw_out), bytes(pre)


def _defined(pvk, raw, pre, inputs, n, n_public, flags):
    """The status bytes of the definition: the raw batch on the GPU, MALFORMED where pre is set."""
    st = pvk.verify_batch(raw, inputs, n, 256, n_public, flags=flags)
    return bytes(6 if pre[i] else st[i] for i in range(n))


def _pad(recs, n, stride):
    return b"".join(recs[128 * i:128 * (i + 1)] + bytes([0x5A]) * (stride - 128) for i in range(n))


@pytest.mark.parametrize("n_public,n", [(2, 4096), (17, 700), (1024, 160)])
def test_host_entry_matches_definition(pkg, O, L, n_public, n):
    vk, proofs, inputs, exp = pkg.synth_groth16(0xC0C00000 + n_public, n_public, n, invalid_every=7, agree=True, threads=16)
    pvk = pkg.PreparedVk(vk)
    try:
        recs, raw, pre = _compress_batch(pkg, proofs, n, n_public, invalid_every=7)
        want = _defined(pvk, raw, pre, inputs, n, n_public, 0)
        assert pre.count(1) > n // 20 and set(want) >= {pkg.ACCEPT, pkg.REJECT, pkg.ERR_MALFORMED, pkg.ERR_NOT_IN_SUBGROUP}
        assert pvk.verify_batch(recs, inputs, n, n_public=n_public, compressed=True) == want
        for stride in (131, 324):
            assert pvk.verify_batch(_pad(recs, n, stride), inputs, n, stride, n_public, compressed=True) == want
        assert pvk.verify_batch_multi(recs, inputs, 1, n, n_public=n_public, compressed=True) == want
        # strict scalars: the raw path's answer on the decompressed records, MALFORMED still first
        bad_in = bytearray(inputs)
        for i in range(0, n, 5):
            bad_in[32 * n_public * i:32 * n_public * i + 32] = b"\xff" * 32
        want_s = _defined(pvk, raw, pre, bytes(bad_in), n, n_public, pkg.FLAG_STRICT_SCALARS)
        assert pvk.verify_batch(recs, bytes(bad_in), n, n_public=n_public, flags=pkg.FLAG_STRICT_SCALARS, compressed=True) == want_s
        assert pkg.ERR_NOT_MEMBER in want_s
        # a sample against the oracle (the oracle reads raw records; the sample avoids the records that do not decompress)
        idx = [i for i in range(0, n, max(1, n // 16)) if not pre[i]][:12]
        row = 32 * n_public
        sp, si = b"".join(raw[256 * j:256 * (j + 1)] for j in idx), b"".join(inputs[row * j:row * (j + 1)] for j in idx)
        assert O.groth16_verify_many(sp, 256, vk, si, n_public, len(idx)) == bytes(want[j] for j in idx)
    finally:
        pvk.close()


def test_input_len_loses_to_malformed(pkg, L):
    n_public, n = 2, 600
    vk, proofs, inputs, exp = pkg.synth_groth16(0xC0C01000, n_public, n, invalid_every=0, agree=True, threads=16)
    pvk = pkg.PreparedVk(vk)
    try:
        recs, raw, pre = _compress_batch(pkg, proofs, n, 3)
        ins = bytes(32 * 3 * n)
        got = pvk.verify_batch(recs, ins, n, n_public=3, compressed=True)
        assert got == bytes(pkg.ERR_MALFORMED if pre[i] else pkg.ERR_INPUT_LEN for i in range(n))
    finally:
        pvk.close()


def _device_run(pkg, pvk, recs, inputs, n, n_public, stride, flags):
    import torch
    dev = torch.device("cuda:0")
    dp = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    di = torch.frombuffer(bytearray(inputs), dtype=torch.uint8).to(dev)
    ds = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    torch.cuda.synchronize(dev)
    pvk.verify_batch_device(dp.data_ptr(), di.data_ptr(), ds.data_ptr(), n, stride, n_public, 0, s.cuda_stream, flags=flags, compressed=True)
    s.synchronize()
    return bytes(ds.cpu().numpy().tobytes())


@pytest.mark.parametrize("n", [65536, (1 << 20) + 4099])
def test_device_entry_lane_range_and_two_chunks(pkg, L, n):
    """The lane kernels (65 536: two sub-batch streams) and a batch of two workspace chunks, so two decompression chunks over one scratch."""
    n_public = 2
    vk, proofs, inputs, exp = pkg.synth_groth16(0xC0C02000, n_public, n, invalid_every=97, agree=True, threads=32)
    pvk = pkg.PreparedVk(vk)
    try:
        recs, raw, pre = _compress_batch(pkg, proofs, n, 5, bad_every=1013, invalid_every=97)
        want = _defined(pvk, raw, pre, inputs, n, n_public, 0)
        assert _device_run(pkg, pvk, recs, inputs, n, n_public, 128, 0) == want
    finally:
        pvk.close()


@pytest.mark.parametrize("n_public,n", [(2, 4096), (17, 2048)])
def test_rlc_with_malformed_records_in_groups(pkg, L, n_public, n):
    pkg.set_rlc_params(min_batch=64, adaptive=0)
    try:
        vk, proofs, inputs, exp = pkg.synth_groth16(0xC0C03000 + n_public, n_public, n, invalid_every=0, agree=True, threads=16)
        pvk = pkg.PreparedVk(vk)
        try:
            recs, raw, pre = _compress_batch(pkg, proofs, n, 7, bad_every=53)
            want = _defined(pvk, raw, pre, inputs, n, n_public, 0)
            assert pvk.rlc_state()[0] == -1.0
            assert pvk.verify_batch(recs, inputs, n, n_public=n_public, flags=pkg.FLAG_RLC, compressed=True) == want
            share = pvk.rlc_state()[0]
            assert share != -1.0                          # the mode ran
            # a record that does not decompress is no longer pending: it does not send its group to the exact fallback.  The only other odd records are
            # the G2-generator ones, which fail their equation and do
            gen = sum(1 for i in range(n) if not pre[i] and want[i] != pkg.ACCEPT)
            assert share * n <= 40 * gen + 1, (share, gen)
            assert _device_run(pkg, pvk, recs, inputs, n, n_public, 128, pkg.FLAG_RLC) == want
        finally:
            pvk.close()
    finally:
        pkg.set_rlc_params(min_batch=200000, adaptive=1)


def test_reference_mode_key_takes_gnark_root_order(pkg, L):
    """A BN254_VK_REFERENCE key: proofs whose B roots order differently by c0 and lexicographically still ACCEPT (proof points use gnark's order)."""
    import ctypes as C
    n_public, n = 2, 256
    vk, proofs, inputs, exp = pkg.synth_groth16(0xC0C04000, n_public, n, invalid_every=0, agree=True, threads=16)
    pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
    try:
        recs = b"".join(pkg.compress_proof(proofs[256 * i:256 * (i + 1)]) for i in range(n))
        st = C.c_uint8(); o0 = (C.c_uint8 * 128)(); o1 = (C.c_uint8 * 128)()
        disagree = []
        for i in range(n):
            b = recs[128 * i + 32:128 * i + 96]
            L.bn254_g2_decompress(b, o0, 0, 0, C.byref(st)); L.bn254_g2_decompress(b, o1, 1, 0, C.byref(st))
            if bytes(o0) != bytes(o1):
                disagree.append(i)
        assert len(disagree) > 10
        got = pvk.verify_batch(recs, inputs, n, n_public=n_public, compressed=True)
        assert got == bytes([pkg.ACCEPT]) * n
    finally:
        pvk.close()


def test_sp1_groth16_fixtures_compressed(pkg, O, fixtures, L):
    """The four SP1 Groth16 fixtures, compressed: the same verdict as their raw bytes and the oracle's (their verifying key is not among the fixtures, so the
    key is a synthetic one and the verdict is REJECT), at strides 128 and 324."""
    fx, _ = fixtures
    vk, _, _, _ = pkg.synth_groth16(0xC0C05000, 2, 1, invalid_every=0, agree=True)
    pvk = pkg.PreparedVk(vk)
    try:
        seen = 0
        for name, f in sorted(fx.items()):
            if f["variant"] != "groth16":
                continue
            raw = bytes.fromhex(f["raw_proof"])
            pis = b"".join(int(x).to_bytes(32, "big") for x in f["public_inputs"])
            c = pkg.compress_proof(raw[:256])
            want = pvk.verify_batch(raw, pis, 1, proof_stride=len(raw))
            assert want == bytes([O.groth16_verify(raw, vk, [int(x) for x in f["public_inputs"]])]) == bytes([pkg.REJECT]), name
            assert pvk.verify_batch(c, pis, 1, compressed=True) == want, name
            assert pvk.verify_batch(c + bytes(196), pis, 1, proof_stride=324, compressed=True) == want, name
            seen += 1
        assert seen == 4
    finally:
        pvk.close()
