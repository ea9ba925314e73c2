"""SP1 proofs from their public values, on the CPU: the digest rule pinned by the SP1 fixtures and by hashlib, the host compile of k_sp1_public_inputs's body
(bn254_dbg_sp1_public_inputs, device -1: csrc/bn254_sha256.h) over every length, alignment and range case, the argument rules of the four batch entries (all
refused before any device is touched), and the synthetic prover for chosen inputs against the oracle."""
import ctypes as C
import hashlib
import os
import random

import pytest

import sp1_data as S

BAD = -1   # BN254_E_BAD_ARG


def _expected_rows(vkh, stride, pv, offs, pv_bytes):
    rows, bad = [], []
    for i in range(len(offs) - 1):
        h = vkh[i * stride:i * stride + 32]
        o0, o1 = offs[i], offs[i + 1]
        ok = o0 <= o1 <= pv_bytes
        rows.append(h + S.digest(pv[o0:o1] if ok else b""))
        bad.append(0 if ok else 1)
    return b"".join(rows), bytes(bad)


def test_digest_pins_the_sp1_fixtures(pkg):
    """For all eight fixture files: the digest of the public values (parsed from the bincode here) is public input 1 as bn254_sp1_fixture_parse reads it
    (input 0 is the program's vkey hash; the 32 bytes after the raw proof are the circuit key's hash, not an input).  The three distinct digests have top bits 7, 5 and 2, so the mask is exercised."""
    L = pkg.lib()
    tops = set()
    for name in S.NAMES:
        for kind in ("plonk", "groth16"):
            buf = open(os.path.join(S.GOLDEN, "%s_%s_proof.bin" % (name, kind)), "rb").read()
            variant, raw, inputs, vkh, pv = S.parse(buf)
            v = C.c_int(0); rp = (C.c_uint8 * 2048)(); rl = C.c_size_t(0); pis = (C.c_uint8 * 64)(); h = (C.c_uint8 * 32)()
            assert L.bn254_sp1_fixture_parse(buf, C.c_size_t(len(buf)), C.byref(v), rp, C.c_size_t(2048), C.byref(rl), pis, h) == 0
            assert bytes(pis) == inputs and bytes(h) == vkh and bytes(rp)[:rl.value] == raw
            assert pkg.sp1_public_values_digest(pv) == bytes(pis)[32:]
            tops.add(hashlib.sha256(pv).digest()[0] >> 5)
    assert tops == {7, 5, 2}


def test_digest_against_hashlib():
    import importlib
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    rng = random.Random(1)
    for n in list(range(0, 301)) + [1000, 4096, 65536, 1 << 20]:
        m = rng.randbytes(n)
        assert pkg.sp1_public_values_digest(m) == S.digest(m), n


@pytest.mark.parametrize("stride", [0, 32, 40])
def test_host_compile_every_length_and_alignment(pkg, stride):
    """Every length 0..1030 at every start offset mod 16, in one buffer; the vkey hashes include values >= r and 2^256 - 1, which pass through unchanged."""
    rng = random.Random(stride)
    lengths = list(range(0, 1031))
    vals, offs, pos = [], [], 0
    buf = bytearray()
    for k, n in enumerate(lengths):
        pad = (k % 16 - len(buf)) % 16           # start offset k mod 16
        buf += rng.randbytes(pad)
        offs.append(len(buf))
        buf += rng.randbytes(n)
    offs.append(len(buf))
    # contiguous ranges: proof i is [offs[i], offs[i+1]) -- so lengths include the padding; that is fine, every (length, alignment) still occurs
    n = len(offs) - 1
    hs = [rng.randbytes(32) for _ in range(n)]
    hs[0] = S.R.to_bytes(32, "big"); hs[1] = b"\xff" * 32; hs[2] = (S.R + 5).to_bytes(32, "big")
    if stride == 0:
        vkh = hs[0]
    else:
        vkh = b"".join(h + rng.randbytes(stride - 32) for h in hs)
    rows, bad = pkg.dbg_sp1_public_inputs(vkh, stride, bytes(buf), offs)
    erows, ebad = _expected_rows(vkh if stride else vkh, stride, bytes(buf), offs, len(buf))
    assert bad == ebad == bytes(n)
    assert rows == erows


def test_host_compile_exact_lengths_at_every_alignment(pkg):
    """Ranges that are exactly each length (not contiguous): length 0..1030 x start offset 0..15, and the ends of the buffer (a range that ends at
    pv_bytes, one that starts at 0)."""
    rng = random.Random(7)
    buf = rng.randbytes(1100)
    offs_pairs = [(s, s + n) for n in range(0, 1031) for s in (n % 16, 16 + (n * 7) % 16)]
    offs_pairs += [(1100 - n, 1100) for n in range(0, 80)] + [(0, n) for n in range(0, 80)]
    # non-contiguous: one call per pair set through the offset array trick -- proof i uses offsets [2i, 2i+1], so pass a call per pair
    flat = []
    for a, b in offs_pairs:
        flat += [a, b]
    # a single call with ranges [a, b) as proofs 0, 2, 4, ... ; the odd proofs are the (possibly decreasing) gaps between them
    rows, bad = pkg.dbg_sp1_public_inputs(b"\x07" * 32, 0, buf, flat)
    erows, ebad = _expected_rows(b"\x07" * 32, 0, buf, flat, len(buf))
    assert rows == erows and bad == ebad
    assert all(bad[2 * i] == 0 for i in range(len(offs_pairs)))


def test_host_compile_flags_bad_ranges(pkg):
    buf = bytes(range(256)) * 2
    offs = [0, 10, 5, 600, 512, 512, 513, 0]   # [0,10) ok; [10,5) decreasing; [5,600) past; [600,512) decreasing; [512,512) ok (empty, at the end); [512,513) past; [513,0)
    rows, bad = pkg.dbg_sp1_public_inputs(b"\x01" * 32, 0, buf, offs, pv_bytes=512)
    assert list(bad) == [0, 1, 1, 1, 0, 1, 1]
    erows, ebad = _expected_rows(b"\x01" * 32, 0, buf, offs, 512)
    assert rows == erows and bad == ebad
    # pv_bytes smaller than the buffer: nothing past it is read, the range is flagged
    rows, bad = pkg.dbg_sp1_public_inputs(b"\x01" * 32, 0, buf, [0, 100, 101], pv_bytes=100)
    assert list(bad) == [0, 1]


def test_row_scratch_sizing(pkg):
    """bn254_g16_plan.h::g16_sp1_alloc through its probe: whole 256-proof units up to the chunk of 2^20 proofs and no more (larger batches are hashed chunk by
    chunk), 64 bytes of row per proof, the pre bytes right after the rows (a multiple of 256 proofs, so they start 16 KiB-aligned), one per proof."""
    L = pkg.lib()
    L.bn254_dbg_g16_sp1_alloc.argtypes = [C.c_size_t, C.c_void_p]
    out = (C.c_uint64 * 3)()
    chunk = 1 << 20
    for n in [0, 1, 255, 256, 257, 4096, 65535, 65536, chunk - 1, chunk, chunk + 1, chunk + 777, 3 * chunk, 1 << 40]:
        assert L.bn254_dbg_g16_sp1_alloc(n, C.cast(out, C.c_void_p)) == 0
        proofs, row_bytes, pre_bytes = out
        assert proofs == min(-(-n // 256) * 256, chunk), n
        assert proofs % 256 == 0 and proofs >= min(n, chunk)
        assert row_bytes == 64 * proofs and row_bytes % (64 * 256) == 0
        assert pre_bytes == proofs
    assert L.bn254_dbg_g16_sp1_alloc(1, None) == BAD


def _g16_key(pkg):
    L = pkg.lib()
    vk, proofs, inputs, _ = pkg.synth_groth16(7, 2, 1, invalid_every=0, agree=True)
    h = C.c_void_p()
    assert L.bn254_groth16_vk_prepare(vk, len(vk), 1, C.byref(h)) == 0
    return h, proofs


def test_argument_rules(pkg):
    """Every argument error is BN254_E_BAD_ARG before any device is touched (this machine has none: a call that got as far as a device would answer
    BN254_E_NO_DEVICE); n = 0 is OK."""
    L = pkg.lib()
    g, proofs = _g16_key(pkg)
    pvk_bytes = open(os.path.join(os.path.dirname(S.GOLDEN), "plonk_vk.bin"), "rb").read()
    p = C.c_void_p()
    assert L.bn254_plonk_vk_prepare(pvk_bytes, len(pvk_bytes), C.byref(p)) == 0
    vp = C.c_void_p
    host = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    dev = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_int, vp, C.c_uint]
    L.bn254_sp1_groth16_verify_batch.argtypes = host
    L.bn254_sp1_plonk_verify_batch.argtypes = host
    L.bn254_sp1_groth16_verify_batch_device.argtypes = dev
    L.bn254_sp1_plonk_verify_batch_device.argtypes = dev
    try:
        n = 4
        st = (C.c_uint8 * n)()
        pv, offs = pkg.sp1_pack_values([b"a", b"bc", b"", b"def"])
        offp = C.cast(offs, C.c_void_p)
        vkh = bytes(32 * n)
        down = (C.c_uint64 * 5)(0, 1, 3, 2, 6)
        for kind, h, recs, stride, fl_ok in (("groth16", g, proofs * n, 256, 0), ("plonk", p, bytes(904 * n), 904, 0)):
            H = getattr(L, "bn254_sp1_%s_verify_batch" % kind)
            D = getattr(L, "bn254_sp1_%s_verify_batch_device" % kind)
            # NULL pointers with n > 0
            assert H(h, None, stride, vkh, 32, pv, offp, n, st, 0, 0) == BAD
            assert H(h, recs, stride, None, 32, pv, offp, n, st, 0, 0) == BAD
            assert H(h, recs, stride, vkh, 32, None, offp, n, st, 0, 0) == BAD
            assert H(h, recs, stride, vkh, 32, pv, None, n, st, 0, 0) == BAD
            assert H(h, recs, stride, vkh, 32, pv, offp, n, None, 0, 0) == BAD
            assert H(None, recs, stride, vkh, 32, pv, offp, n, st, 0, 0) == BAD
            assert D(h, None, stride, vkh, 32, pv, len(pv), offp, n, st, 0, None, 0) == BAD
            assert D(h, recs, stride, None, 32, pv, len(pv), offp, n, st, 0, None, 0) == BAD
            assert D(h, recs, stride, vkh, 32, None, len(pv), offp, n, st, 0, None, 0) == BAD
            assert D(h, recs, stride, vkh, 32, pv, len(pv), None, n, st, 0, None, 0) == BAD
            assert D(h, recs, stride, vkh, 32, pv, len(pv), offp, n, None, 0, None, 0) == BAD
            # vkey_stride 1..31
            for vs in range(1, 32):
                assert H(h, recs, stride, vkh, vs, pv, offp, n, st, 0, 0) == BAD
                assert D(h, recs, stride, vkh, vs, pv, len(pv), offp, n, st, 0, None, 0) == BAD
            # decreasing host offsets
            assert H(h, recs, stride, vkh, 32, pv, C.cast(down, C.c_void_p), n, st, 0, 0) == BAD
            # unknown flags
            assert H(h, recs, stride, vkh, 32, pv, offp, n, st, 0, 8) == BAD
            assert D(h, recs, stride, vkh, 32, pv, len(pv), offp, n, st, 0, None, 8) == BAD
            # n = 0
            assert H(h, recs, stride, vkh, 32, pv, offp, 0, st, 0, 0) == 0
            assert D(h, recs, stride, vkh, 0, pv, len(pv), offp, 0, st, 0, None, 0) == 0
        # the PlonK entries given STRICT or COMPRESSED
        for fl in (1, 4, 1 | 2):
            assert L.bn254_sp1_plonk_verify_batch(p, bytes(904 * n), 904, vkh, 32, pv, offp, n, st, 0, fl) == BAD
            assert L.bn254_sp1_plonk_verify_batch_device(p, bytes(904 * n), 904, vkh, 32, pv, len(pv), offp, n, st, 0, None, fl) == BAD
        # Groth16 stride rules as the raw entry: 255 raw, 127 compressed
        assert L.bn254_sp1_groth16_verify_batch(g, proofs * n, 255, vkh, 32, pv, offp, n, st, 0, 0) == BAD
        assert L.bn254_sp1_groth16_verify_batch(g, proofs * n, 127, vkh, 32, pv, offp, n, st, 0, 4) == BAD
        # well-formed calls get past the check: on a machine without a GPU they stop at the device
        rc = L.bn254_sp1_groth16_verify_batch(g, proofs * n, 256, vkh, 32, pv, offp, n, st, 0, 0)
        assert rc != BAD
    finally:
        L.bn254_groth16_vk_free(g)
        L.bn254_plonk_vk_free(p)


def test_synth_for_inputs_against_the_oracle(pkg, O):
    """64 proofs for random inputs, some of them >= r: all ACCEPT under the oracle; one mutated input gives REJECT; the key is synth_groth16's."""
    rng = random.Random(3)
    n, n_public = 64, 2
    rows = []
    for i in range(n):
        for s in range(n_public):
            x = rng.getrandbits(256) if i % 4 == 0 else rng.randrange(S.R)
            rows.append(x.to_bytes(32, "big"))
    assert any(int.from_bytes(r, "big") >= S.R for r in rows)
    inputs = b"".join(rows)
    vk, proofs = pkg.synth_groth16_for_inputs(0x5B1, n_public, inputs)
    vk2, _, _, _ = pkg.synth_groth16(0x5B1, n_public, 1, invalid_every=0, agree=True)
    assert vk == vk2
    st = O.groth16_verify_many(proofs, 256, vk, inputs, n_public, n, O.MODE_REFERENCE)
    assert st == bytes([pkg.ACCEPT] * n)
    bad = bytearray(inputs); bad[32 * 5 + 31] ^= 1
    st = O.groth16_verify_many(proofs, 256, vk, bytes(bad), n_public, n, O.MODE_REFERENCE)
    assert st[2] == pkg.REJECT and st[:2] + st[3:] == bytes([pkg.ACCEPT] * (n - 1))
