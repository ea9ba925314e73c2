"""Compaction of the lane launches of the exact Groth16 path (csrc/bn254_g16_plan.h: g16_compacts, g16_compact_alloc, g16_compact_partial), without a GPU.

The plan: which launches compact, and that the slots and block counts every such launch addresses lie inside what the context allocates beside its workspace,
disjoint between launches that run side by side -- a walk over keys, reservations, batch sizes and flags in the style of
tests/test_capi_cpu.py::test_groth16_plan_fits_every_reservation.  The count -> scan -> write step: the host restatement (bn254_dbg_g16_compact, whose scan is the
function k_g16_compact_write runs) against a plain Python compaction for random pending masks, the all-zero and the all-one mask among them."""
import ctypes as C
import random

COOP, WIDE_MIN, MAXB, MAXL = 30720, 16, 1 << 20, 786432
NO_PROOF, PENDING = 0xFFFFFFFF, 0x80


def _compact_plan(L, key_inputs, reserved, n, n_public, flags, n_streams, single):
    L.bn254_dbg_g16_compact_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.c_int, C.POINTER(C.c_int)]
    alloc = (C.c_uint64 * 3)(); out = (C.c_uint64 * (6 * 64))(); k = C.c_int()
    assert L.bn254_dbg_g16_compact_plan(key_inputs, reserved, n, n_public, flags, n_streams, single, alloc, out, 64, C.byref(k)) == 0
    assert k.value <= 64
    return [int(x) for x in alloc], [[int(out[6 * i + j]) for j in range(6)] for i in range(k.value)]


def test_compaction_plan_and_reservation(pkg):
    """A launch compacts exactly when it is a lane launch (form 0: above the cooperative hand-over, or a part of a larger batch) of a key with at most 16 inputs in a
    call with neither STRICT_SCALARS nor RLC; the context of such a key holds 4 + 1 bytes per workspace proof and one count per 256, a key with more inputs none;
    every launch that compacts stays inside them, and the launches of a chunk use disjoint slots and counts."""
    L = pkg.lib()
    rng = random.Random(0xC0A7)
    sizes = [1, 255, 256, 257, 4096, 30720, 30721, 30800, 65536, 65537, 65552, 131072, 524288, 786432, 786433, (1 << 20) - 1, 1 << 20, (1 << 20) + 777, 2500000]
    seen_compact = seen_plain = 0
    for key_inputs in (0, 2, 16, 17, 40):
        for reserved in sizes + [rng.randrange(1, 1 << 21) for _ in range(4)]:
            ws_proofs = min((reserved + 255) // 256 * 256, MAXB)
            for n in {reserved, max(1, reserved // 2), max(1, reserved - 1), min(reserved, 70000), min(reserved, 30721)}:
                for n_public in {key_inputs, max(0, key_inputs - 1)}:
                    for flags in (0, pkg.FLAG_STRICT_SCALARS, pkg.FLAG_RLC, pkg.FLAG_RLC | pkg.FLAG_STRICT_SCALARS):
                        for n_streams, single in ((2, 0), (1, 0), (4, 0), (2, 1)):
                            alloc, rows = _compact_plan(L, key_inputs, reserved, n, n_public, flags, n_streams, single)
                            if key_inputs <= WIDE_MIN:
                                assert alloc == [4 * ws_proofs, ws_proofs, 4 * (ws_proofs // 256)], (key_inputs, reserved, alloc)
                            else:
                                assert alloc == [0, 0, 0]
                            pos = covered = 0
                            for r, (compacts, first, count, first_block, blocks, form) in enumerate(rows):
                                covered += count
                                assert compacts == int(form == 0 and key_inputs <= WIDE_MIN and flags == 0), (key_inputs, n, n_public, flags, rows)
                                if form == 0 and len(rows) == 1:
                                    assert count > COOP or n_public > WIDE_MIN       # a whole batch in the lane form: above the cooperative hand-over
                                if first == 0:
                                    pos = 0                                            # a new workspace chunk: its launches reuse the slots of the chunk before it
                                assert first == pos                                    # the parts of a chunk follow each other
                                pos = first + count
                                if not compacts:
                                    seen_plain += 1
                                    continue
                                seen_compact += 1
                                padded = (count + 255) // 256 * 256                    # the grid of the launch: whole blocks of 256 slots
                                last_of_chunk = r + 1 == len(rows) or rows[r + 1][1] == 0
                                assert count <= MAXL and first % 256 == 0 and first_block == first // 256 and blocks == padded // 256
                                assert count % 256 == 0 or last_of_chunk               # so the blocks of one part never reach into the next part's slots
                                assert 4 * (first + padded) <= alloc[0] and first + padded <= alloc[1] and 4 * (first_block + blocks) <= alloc[2]
                            assert covered == n
    assert seen_compact > 1000 and seen_plain > 1000


def _host_compact(L, mask):
    n = len(mask)
    L.bn254_dbg_g16_compact.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    sp = (C.c_uint32 * n)(*([0xDEADBEEF] * n)); ss = (C.c_uint8 * n)(*([0xEE] * n)); k = C.c_uint32(0xDEADBEEF)
    assert L.bn254_dbg_g16_compact(bytes(mask), n, sp, ss, C.byref(k)) == 0
    return list(sp), bytes(ss), k.value


def test_count_scan_write_is_a_stable_compaction(pkg):
    """slot_proof lists the pending proofs in order, slot_status is PENDING on that list and 0 after it, for masks of every density and for sizes around the block of
    256, one block, many blocks, a ragged last block and the largest launch's 3072 counts"""
    L = pkg.lib()
    rng = random.Random(0x5CA9)
    cases = []
    for n in (1, 63, 64, 255, 256, 257, 511, 1000, 4097, 30800, 65552):
        cases += [bytes(n), bytes([1]) * n, bytes(rng.randrange(2) for _ in range(n)), bytes(int(rng.random() < 1 / 40) for _ in range(n)),
                  bytes(int(rng.random() > 1 / 40) for _ in range(n))]
    cases += [bytes(int(i % 256 != 0) for i in range(5000)), bytes(int(i % 256 != 255) for i in range(5000)), bytes(int(not 256 <= i < 512) for i in range(1500)),
              bytes(int(i < 1024) for i in range(1100)), bytes(int(i >= 64) for i in range(300))]
    cases.append(bytes(int(rng.random() > 1 / 40) for _ in range(MAXL)))
    for mask in cases:
        n = len(mask)
        want = [i for i in range(n) if mask[i]]
        sp, ss, k = _host_compact(L, mask)
        assert k == len(want)
        assert sp[:k] == want
        assert ss == bytes([PENDING]) * k + bytes(n - k)
        assert all(x == NO_PROOF for x in sp[k:])
    L.bn254_dbg_g16_compact.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.bn254_dbg_g16_compact(b"\x01", 0, None, None, None) != 0
