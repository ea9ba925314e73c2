"""GPU tests of the SP1 entries (k_sp1_public_inputs, then the unchanged Groth16 / PlonK pipeline with n_public = 2, then the MALFORMED merge): the device
digests byte for byte against hashlib; every status byte of the Groth16 and PlonK SP1 entries equal to the raw entry's on hashlib-computed inputs
vkey_hash | digest (the definition of include/bn254_verify.h), across mutations of values, vkey hashes and proofs, BN254_FLAG_RLC / STRICT_SCALARS /
COMPRESSED_PROOFS, vkey strides 0 and 32, a batch that crosses a workspace chunk, a key of the wrong width, the real SP1 PlonK fixtures and two threads on one
key; bad ranges on the device entries; samples against the oracle."""
import os
import random
import threading

import pytest

import sp1_data as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def rlc_every_call(pkg):
    """BN254_FLAG_RLC honoured from 64 proofs and never bypassed (the adaptive bypass would send a call after a batch with many failed groups to the exact path);
    the defaults the other test files rely on are restored afterwards."""
    pkg.set_rlc_params(min_batch=64, adaptive=0)
    try:
        yield
    finally:
        pkg.set_rlc_params(min_batch=200000, adaptive=1)


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


def _d(torch_dev, b):
    torch, dev = torch_dev
    b = bytes(b)
    return torch.frombuffer(bytearray(b if b else b"\0"), dtype=torch.uint8).to(dev)


def _d_u64(torch_dev, xs):
    torch, dev = torch_dev
    return torch.tensor(list(xs), dtype=torch.int64).to(dev)


def _offsets(values):
    offs, acc = [0], 0
    for v in values:
        acc += len(v)
        offs.append(acc)
    return offs


def _rows(vkhs, values):
    return b"".join(h + S.digest(v) for h, v in zip(vkhs, values))


# ---------------------------------------------------------------------------------------------------------------------------------- device digests
def test_device_digests(pkg):
    """70 000 records through the kernel: every length 0..1030, the rest random up to 2 KiB, unaligned starts, one 1 MiB value, bad ranges flagged."""
    rng = random.Random(11)
    lens = list(range(0, 1031)) + [rng.randrange(0, 2049) for _ in range(70000 - 1031 - 1)] + [1 << 20]
    buf = bytearray()
    pairs = []
    for k, n in enumerate(lens):
        buf += rng.randbytes(rng.randrange(0, 16))      # unaligned starts
        pairs.append((len(buf), len(buf) + n))
        buf += rng.randbytes(n)
    buf = bytes(buf)
    # proof i = [offs[i], offs[i+1]): contiguous ranges covering the gaps too, plus a few bad ones at the end
    offs = [pairs[0][0]] + [b for _, b in pairs]
    offs += [len(buf) - 3, len(buf) + 1, 17, len(buf)]   # after the last offset len(buf): decreasing, past the end, decreasing, ok
    n = len(offs) - 1
    vkhs = [rng.randbytes(32) for _ in range(n)]
    rows, bad = pkg.dbg_sp1_public_inputs(b"".join(vkhs), 32, buf, offs, device=0)
    for i in range(n):
        o0, o1 = offs[i], offs[i + 1]
        ok = o0 <= o1 <= len(buf)
        assert bad[i] == (0 if ok else 1), i
        assert rows[64 * i:64 * i + 64] == vkhs[i] + S.digest(buf[o0:o1] if ok else b""), i
    assert list(bad[-4:]) == [1, 1, 1, 0] and sum(bad) == 3


# ---------------------------------------------------------------------------------------------------------------------------------- Groth16
class G16Set:
    """A synthetic 2-input key and n proofs made for vkh_i | digest(pv_i); vkh_i >= r for i = 5 mod 37 (the proof is made for it mod r)."""

    def __init__(self, pkg, n, seed, one_vkh=False):
        rng = random.Random(seed)
        self.n = n
        self.one_vkh = one_vkh
        if one_vkh:
            self.vkhs = [rng.randrange(S.R).to_bytes(32, "big")] * n
        else:
            self.vkhs = [((S.R + rng.randrange(1 << 250)) if i % 37 == 5 else rng.randrange(S.R)).to_bytes(32, "big") for i in range(n)]
        self.values = [rng.randbytes(96 if i % 3 else rng.randrange(0, 300)) for i in range(n)]
        self.vk, self.proofs = pkg.synth_groth16_for_inputs(0x5B100 + seed, 2, _rows(self.vkhs, self.values), threads=16)

    def mutated(self, rng, every=16):
        """Every `every`-th proof mutated in turn: value byte flipped, byte appended, byte dropped, vkey hash changed (a value byte flipped when the batch has one
        vkey hash), A.y + 1, C replaced."""
        vkhs, values, proofs = list(self.vkhs), list(self.values), bytearray(self.proofs)
        kinds = []
        for k, i in enumerate(range(every - 1, self.n, every)):
            kind = k % 6
            if kind == 3 and self.one_vkh:
                kind = 0
            v = values[i]
            if kind == 0:
                values[i] = (bytes([v[0] ^ 1]) + v[1:]) if v else b"\x01"
            elif kind == 1:
                values[i] = v + b"\x00"
            elif kind == 2:
                values[i] = v[:-1] if v else b"\x00"
            elif kind == 3:
                vkhs[i] = bytes([vkhs[i][0]]) + bytes([vkhs[i][1] ^ 0x40]) + vkhs[i][2:]
            elif kind == 4:
                y = int.from_bytes(proofs[256 * i + 32:256 * i + 64], "big") + 1
                proofs[256 * i + 32:256 * i + 64] = (y % (1 << 256)).to_bytes(32, "big")
            else:
                proofs[256 * i + 192:256 * i + 256] = self.proofs[256 * ((i + 1) % self.n) + 192:256 * ((i + 1) % self.n) + 256]
            kinds.append(i)
        return vkhs, values, bytes(proofs), kinds


def _g16_run_all(pkg, torch_dev, pvk, proofs, vkhs, values, flags=0, stride=256, one_vkh=False, device_only=False, sp1_keys=None):
    """(raw device statuses on hashlib inputs, SP1 device statuses, SP1 host statuses).  sp1_keys: (device entry's key, host entry's key), default pvk."""
    sp1_dev_key, sp1_host_key = sp1_keys or (pvk, pvk)
    torch, dev = torch_dev
    n = len(values)
    rows = _rows(vkhs, values)
    stream = torch.cuda.current_stream(dev)
    d_p, d_r = _d(torch_dev, proofs), _d(torch_dev, rows)
    d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    pvk.verify_batch_device(d_p.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), n, proof_stride=stride, n_public=2, stream=stream.cuda_stream, flags=flags)
    stream.synchronize()
    raw = bytes(d_s.cpu().numpy().tobytes())
    pv = b"".join(values)
    d_v, d_o = _d(torch_dev, pv), _d_u64(torch_dev, _offsets(values))
    vk_arg = vkhs[0] if one_vkh else b"".join(vkhs)
    d_h = _d(torch_dev, vk_arg)
    d_s2 = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    sp1_dev_key.verify_sp1_batch_device(d_p.data_ptr(), d_h.data_ptr(), d_v.data_ptr(), len(pv), d_o.data_ptr(), d_s2.data_ptr(), n, proof_stride=stride,
                                        vkey_stride=0 if one_vkh else 32, stream=stream.cuda_stream, flags=flags)
    stream.synchronize()
    sp1_dev = bytes(d_s2.cpu().numpy().tobytes())
    sp1_host = None if device_only else sp1_host_key.verify_sp1_batch(proofs, vkhs[0] if one_vkh else vkhs, values, proof_stride=stride, flags=flags)
    return raw, sp1_dev, sp1_host


def _check_parity(pkg, O, torch_dev, gs, flags=0, seed=1, one_vkh=False, compressed=False, device_only=False):
    rng = random.Random(seed)
    vkhs, values, proofs, mut = gs.mutated(rng)
    stride = 256
    if compressed:
        recs = bytearray()
        for i in range(gs.n):
            try:
                recs += pkg.compress_proof(proofs[256 * i:256 * i + 256])
            except pkg.Bn254Error:
                recs += bytes([0x80]) + bytes(127)     # A off the curve does not compress: a record that does not decompress stands in
        proofs, stride = bytes(recs), 128
        flags |= pkg.FLAG_COMPRESSED_PROOFS
    # with BN254_FLAG_RLC the SP1 calls run on keys of their own, so that their RLC state shows the mode ran for them (a fallback share is recorded only by
    # an RLC pass)
    keys = (pkg.PreparedVk(gs.vk, pkg.VK_REFERENCE), pkg.PreparedVk(gs.vk, pkg.VK_REFERENCE)) if flags & pkg.FLAG_RLC else None
    if keys:
        assert keys[0].rlc_state()[0] == -1.0 and keys[1].rlc_state()[0] == -1.0
    raw, dev, host = _g16_run_all(pkg, torch_dev, gs.pvk, proofs, vkhs, values, flags, stride, one_vkh, device_only, keys)
    if keys:
        assert keys[0].rlc_state()[0] > 0.0 and (device_only or keys[1].rlc_state()[0] > 0.0), "the SP1 calls did not run the RLC mode"
        for k in keys:
            k.close()
    assert dev == raw
    if host is not None:
        assert host == raw
    mset = set(mut)
    strict_big = (flags & pkg.FLAG_STRICT_SCALARS) and not one_vkh
    for i in range(gs.n):
        if i not in mset and not (strict_big and i % 37 == 5):
            assert raw[i] == pkg.ACCEPT, i
    if not compressed and not flags:
        idx = sorted(rng.sample(range(gs.n), 48) + mut[:16])
        sub_p = b"".join(proofs[256 * i:256 * i + 256] for i in idx)
        sub_in = b"".join(vkhs[i] + S.digest(values[i]) for i in idx)
        ref = O.groth16_verify_many(sub_p, 256, gs.vk, sub_in, 2, len(idx), O.MODE_REFERENCE)
        assert bytes(raw[i] for i in idx) == ref
    return raw


@pytest.fixture(scope="module")
def g16_4096(pkg):
    gs = G16Set(pkg, 4096, 1)
    gs.pvk = pkg.PreparedVk(gs.vk, pkg.VK_REFERENCE)
    return gs


@pytest.fixture(scope="module")
def g16_65536(pkg):
    gs = G16Set(pkg, 65536, 2)
    gs.pvk = pkg.PreparedVk(gs.vk, pkg.VK_REFERENCE)
    return gs


def test_g16_parity_4096(pkg, O, torch_dev, g16_4096):
    _check_parity(pkg, O, torch_dev, g16_4096)


def test_g16_parity_4096_strict(pkg, O, torch_dev, g16_4096):
    raw = _check_parity(pkg, O, torch_dev, g16_4096, flags=pkg.FLAG_STRICT_SCALARS, seed=2)
    assert all(raw[i] == pkg.ERR_NOT_MEMBER for i in range(5, 4096, 37) if i % 16 != 15)


def test_g16_parity_4096_rlc(pkg, O, torch_dev, g16_4096):
    _check_parity(pkg, O, torch_dev, g16_4096, flags=pkg.FLAG_RLC, seed=3)


def test_g16_parity_4096_compressed(pkg, O, torch_dev, g16_4096):
    _check_parity(pkg, O, torch_dev, g16_4096, seed=4, compressed=True)
    _check_parity(pkg, O, torch_dev, g16_4096, flags=pkg.FLAG_RLC | pkg.FLAG_STRICT_SCALARS, seed=5, compressed=True)


def test_g16_parity_one_vkey_hash(pkg, O, torch_dev):
    gs = G16Set(pkg, 4096, 6, one_vkh=True)
    gs.pvk = pkg.PreparedVk(gs.vk, pkg.VK_REFERENCE)
    _check_parity(pkg, O, torch_dev, gs, seed=6, one_vkh=True)


def test_g16_parity_65536(pkg, O, torch_dev, g16_65536):
    _check_parity(pkg, O, torch_dev, g16_65536, seed=7)
    _check_parity(pkg, O, torch_dev, g16_65536, flags=pkg.FLAG_RLC, seed=8)


def test_g16_parity_across_a_chunk(pkg, O, torch_dev):
    """2^20 + 777 proofs: the SP1 entries hash and verify in chunks of 2^20."""
    gs = G16Set(pkg, (1 << 20) + 777, 9)
    gs.pvk = pkg.PreparedVk(gs.vk, pkg.VK_REFERENCE)
    _check_parity(pkg, O, torch_dev, gs, seed=9)


def _host_stride40(pkg, fn, handle, proofs, stride, vkhs, values, flags=0):
    """A host SP1 entry with the vkey hashes 40 bytes apart (the library packs them to 32 bytes per proof)."""
    import ctypes as C
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    vk40 = b"".join(h + bytes([0xA5] * 8) for h in vkhs)
    pv, offs = pkg.sp1_pack_values(values)
    n = len(values)
    st = (C.c_uint8 * n)()
    assert fn(handle, proofs, stride, vk40, 40, pv, C.cast(offs, C.c_void_p), n, st, 0, flags) == 0, pkg.lib().bn254_last_error()
    return bytes(st)


def test_g16_host_vkey_stride_40(pkg, torch_dev, g16_4096):
    """Stride 40 through the Groth16 host entry: the vkey hashes are packed on the host through the pinned ring; same bytes as stride 32 and as the raw entry."""
    rng = random.Random(12)
    vkhs, values, proofs, _ = g16_4096.mutated(rng)
    raw, _dev, host32 = _g16_run_all(pkg, torch_dev, g16_4096.pvk, proofs, vkhs, values)
    got = _host_stride40(pkg, pkg.lib().bn254_sp1_groth16_verify_batch, g16_4096.pvk.handle, proofs, 256, vkhs, values)
    assert got == host32 == raw


def test_g16_wrong_width_key(pkg, torch_dev, g16_4096):
    """A 3-input key: every proof is INPUT_LEN, as the raw entry says for n_public = 2."""
    vk3, _, _, _ = pkg.synth_groth16(0x33, 3, 1, invalid_every=0, agree=True)
    pvk = pkg.PreparedVk(vk3, pkg.VK_REFERENCE)
    n = 512
    vkhs, values, proofs = g16_4096.vkhs[:n], g16_4096.values[:n], g16_4096.proofs[:256 * n]
    raw, dev, host = _g16_run_all(pkg, torch_dev, pvk, proofs, vkhs, values)
    assert raw == dev == host == bytes([pkg.ERR_INPUT_LEN] * n)


def test_g16_device_bad_ranges(pkg, torch_dev, g16_4096):
    """Offsets that decrease or pass pv_bytes: exactly those proofs are MALFORMED, every other byte as with good offsets."""
    torch, dev = torch_dev
    gs = g16_4096
    n = 1024
    values = gs.values[:n]
    pv = b"".join(values)
    offs = _offsets(values)
    good = _g16_run_all(pkg, torch_dev, gs.pvk, gs.proofs[:256 * n], gs.vkhs[:n], values, device_only=True)[1]
    bad_offs = list(offs)
    bad_idx = set()
    for i in range(100, n, 97):
        if i % 2:
            bad_offs[i] = bad_offs[i + 1] + 1      # [off[i], off[i+1]) decreasing; proof i - 1 grows (still inside)
            bad_idx.add(i)
        else:
            bad_offs[i + 1] = len(pv) + 5          # past pv_bytes: proof i, and proof i + 1 decreases
            bad_idx.add(i)
            if bad_offs[i + 2] < bad_offs[i + 1]:
                bad_idx.add(i + 1)
    stream = torch.cuda.current_stream(dev)
    d_p, d_h, d_v, d_o = _d(torch_dev, gs.proofs[:256 * n]), _d(torch_dev, b"".join(gs.vkhs[:n])), _d(torch_dev, pv), _d_u64(torch_dev, bad_offs)
    d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    gs.pvk.verify_sp1_batch_device(d_p.data_ptr(), d_h.data_ptr(), d_v.data_ptr(), len(pv), d_o.data_ptr(), d_s.data_ptr(), n, stream=stream.cuda_stream)
    stream.synchronize()
    got = bytes(d_s.cpu().numpy().tobytes())
    changed = {i for i in range(n) if bad_offs[i] != offs[i] or bad_offs[i + 1] != offs[i + 1]}
    for i in range(n):
        if i in bad_idx:
            assert got[i] == pkg.ERR_MALFORMED, i
        elif i not in changed:
            assert got[i] == good[i], i
        else:
            assert got[i] != pkg.ERR_MALFORMED, i


# ---------------------------------------------------------------------------------------------------------------------------------- PlonK
@pytest.fixture(scope="module")
def plonk(pkg, fixtures):
    fx, vk = fixtures
    items = [S.fixture(name, "plonk") for name in S.NAMES]
    return pkg.PreparedPlonkVk(vk), vk, [(raw, inputs[:32], pv) for _v, raw, inputs, _h, pv in items]


def _plonk_raw(pkg, torch_dev, ppvk, proofs, vkhs, values, flags=0):
    torch, dev = torch_dev
    n = len(values)
    d_p, d_r = _d(torch_dev, proofs), _d(torch_dev, _rows(vkhs, values))
    d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    ppvk.verify_batch_device(d_p.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), n, n_public=2, stream=torch.cuda.current_stream(dev).cuda_stream, flags=flags)
    return bytes(d_s.cpu().numpy().tobytes())


def _plonk_sp1_dev(pkg, torch_dev, ppvk, proofs, vkhs, values, flags=0, offs=None):
    torch, dev = torch_dev
    n = len(values)
    pv = b"".join(values)
    d_p, d_h, d_v, d_o = _d(torch_dev, proofs), _d(torch_dev, b"".join(vkhs)), _d(torch_dev, pv), _d_u64(torch_dev, offs or _offsets(values))
    d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    ppvk.verify_sp1_batch_device(d_p.data_ptr(), d_h.data_ptr(), d_v.data_ptr(), len(pv), d_o.data_ptr(), d_s.data_ptr(), n,
                                 stream=torch.cuda.current_stream(dev).cuda_stream, flags=flags)
    return bytes(d_s.cpu().numpy().tobytes())


def _plonk_mutations(items):
    out = []
    for raw, vkh, pv in items:
        out.append((raw, vkh, pv))
        out.append((raw, vkh, (bytes([pv[0] ^ 1]) + pv[1:]) if pv else b"\x01"))   # flip (or a byte where there was none)
        out.append((raw, vkh, pv + b"\x00"))                                           # append
        out.append((raw, vkh, pv[:-1] if pv else b"\x00\x00"))                         # truncate
        out.append((raw, vkh, b""))                                                    # emptied
        out.append((raw, vkh[:31] + bytes([vkh[31] ^ 1]), pv))                         # vkey hash
    return out


def test_plonk_fixtures_and_mutations(pkg, O, torch_dev, plonk):
    ppvk, vk, items = plonk
    proofs = b"".join(r for r, _, _ in items)
    vkhs = [h for _, h, _ in items]; values = [v for _, _, v in items]
    assert ppvk.verify_sp1_batch(proofs, vkhs, values) == bytes([pkg.ACCEPT] * 4)
    assert _plonk_sp1_dev(pkg, torch_dev, ppvk, proofs, vkhs, values) == bytes([pkg.ACCEPT] * 4)
    mut = _plonk_mutations(items)
    proofs = b"".join(r for r, _, _ in mut)
    vkhs = [h for _, h, _ in mut]; values = [v for _, _, v in mut]
    raw = _plonk_raw(pkg, torch_dev, ppvk, proofs, vkhs, values)
    assert ppvk.verify_sp1_batch(proofs, vkhs, values) == raw
    assert _plonk_sp1_dev(pkg, torch_dev, ppvk, proofs, vkhs, values) == raw
    ref = bytes(O.plonk_verify(r, vk, [int.from_bytes(h, "big"), int.from_bytes(S.digest(v), "big")]) for r, h, v in mut)
    assert raw == ref
    assert sum(1 for x in raw if x == pkg.ACCEPT) == 4 + sum(1 for _, _, v in items if not v)   # emptying an empty value changes nothing


def test_plonk_65536(pkg, torch_dev, plonk):
    """A 65 536-proof batch cycling the fixtures, every 8th proof mutated; exact and RLC."""
    ppvk, _vk, items = plonk
    mut = _plonk_mutations(items)
    n = 65536
    sel = [items[i % 4] if i % 8 else mut[(i // 8) % len(mut)] for i in range(n)]
    proofs = b"".join(r for r, _, _ in sel)
    vkhs = [h for _, h, _ in sel]; values = [v for _, _, v in sel]
    for flags in (0, pkg.FLAG_RLC):
        raw = _plonk_raw(pkg, torch_dev, ppvk, proofs, vkhs, values, flags)
        assert all(raw[i] == pkg.ACCEPT for i in range(n) if i % 8)
        assert ppvk.verify_sp1_batch(proofs, vkhs, values, flags=flags) == raw
        assert _plonk_sp1_dev(pkg, torch_dev, ppvk, proofs, vkhs, values, flags) == raw


def test_plonk_host_vkey_stride_40(pkg, torch_dev, plonk):
    """Stride 40 through the PlonK host entry (vkey hashes packed on the host): the raw entry's bytes."""
    ppvk, _vk, items = plonk
    mut = _plonk_mutations(items)
    proofs = b"".join(r for r, _, _ in mut); vkhs = [h for _, h, _ in mut]; values = [v for _, _, v in mut]
    raw = _plonk_raw(pkg, torch_dev, ppvk, proofs, vkhs, values)
    assert _host_stride40(pkg, pkg.lib().bn254_sp1_plonk_verify_batch, ppvk._h, proofs, 904, vkhs, values) == raw


def test_plonk_two_threads_one_key(pkg, torch_dev, plonk):
    ppvk, _vk, items = plonk
    mut = _plonk_mutations(items)
    batches = []
    for t in range(2):
        sel = [mut[(7 * i + t) % len(mut)] for i in range(3000 + 1000 * t)]
        batches.append((b"".join(r for r, _, _ in sel), [h for _, h, _ in sel], [v for _, _, v in sel]))
    expect = [_plonk_raw(pkg, torch_dev, ppvk, *b) for b in batches]
    got = [None, None]

    def run(t):
        for _ in range(3):
            got[t] = ppvk.verify_sp1_batch(*batches[t])
            if got[t] != expect[t]:
                return

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert got == expect


def test_plonk_device_bad_ranges(pkg, torch_dev, plonk):
    ppvk, _vk, items = plonk
    sel = [items[i % 4] for i in range(64)]
    proofs = b"".join(r for r, _, _ in sel); vkhs = [h for _, h, _ in sel]; values = [v for _, _, v in sel]
    offs = _offsets(values)
    total = offs[-1]
    bad = list(offs)
    bad[9] = bad[10] + 3          # proof 9 decreasing (proof 8 grows past its own values but stays inside)
    bad[41] = total + 1           # proof 40 past pv_bytes, proof 41 decreasing? (it starts past the end: bad too)
    got = _plonk_sp1_dev(pkg, torch_dev, ppvk, proofs, vkhs, values, offs=bad)
    good = _plonk_sp1_dev(pkg, torch_dev, ppvk, proofs, vkhs, values)
    assert good == bytes([pkg.ACCEPT] * 64)
    for i in range(64):
        if i in (9, 40, 41):
            assert got[i] == pkg.ERR_MALFORMED, i
        elif i != 8:
            assert got[i] == good[i], i
