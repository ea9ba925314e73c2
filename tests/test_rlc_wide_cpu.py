"""BN254_FLAG_RLC for keys with more than 8 public inputs, on the CPU: the host compile of the group-scalar fold and of the wide group stage
(snark-bn254-verifier_amd/csrc/bn254_rlc.h: rlc_group_scalar, vm_rlc_group_points_wide; probe bn254_dbg_rlc_wide_group) against Python and the oracle,
and the sizing of the wide form's buffers (bn254_g16_plan.h: g16_plan_rlc_chunk / g16_rlc_wide_alloc) against every launch part it places."""
import random
import struct

import pytest

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
LAMBDA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd
G16_MAX_LAUNCH = 786432


def rlc_plan(n, log2_group, log2_share=0):
    """bn254_rlc_plan.h::rlc_plan: (the halves of the fold rounds, groups)."""
    share = 1 << log2_share
    m = (n + share - 1) // share
    half = [m << k for k in range(log2_share - 1, -1, -1)]
    target = max(1, n >> log2_group)
    cur = m
    while cur > target and len(half) < 28:
        cur = (cur + 1) // 2
        half.append(cur)
    return half, cur


def group_of(i, half):
    for h in half:
        if i >= h:
            i -= h
    return i


def _case(rng, n_public, n, dead_every):
    weights, live, rs = b"", b"", []
    for i in range(n):
        k1, k2 = rng.getrandbits(64), rng.getrandbits(64)
        weights += struct.pack("<QQ", k1, k2)
        alive = dead_every == 0 or i % dead_every != 1
        live += bytes([1 if alive else 0])
        rs.append((k1 + k2 * LAMBDA) % R if alive else 0)
    xs = []
    for i in range(n):
        row = []
        for j in range(n_public):
            c = (i * 7 + j) % 5
            row.append((1 << 256) - 1 - j if c == 0 else R + rng.randrange(1 << 200) if c == 1 else rng.randrange(R))   # inputs >= r are used modulo r
        xs.append(row)
    inputs = b"".join(x.to_bytes(32, "big") for row in xs for x in row)
    return weights, live, rs, xs, inputs


def _key(O, rng, n_public):
    g = O.g1_gen()
    return [O.g1_mul(g, rng.randrange(1, R)) for _ in range(n_public + 1)], O.g1_mul(g, rng.randrange(1, R))


@pytest.mark.parametrize("n_public,n,log2_group,log2_share", [(9, 67, 3, 0), (16, 101, 4, 2), (17, 67, 5, 0), (40, 131, 3, 1), (1024, 37, 3, 0)])
def test_group_scalars_and_point(pkg, O, n_public, n, log2_group, log2_share):
    rng = random.Random(1000 + n_public)
    weights, live, rs, xs, inputs = _case(rng, n_public, n, 5)
    kpts, alpha = _key(O, rng, n_public)
    half, groups = rlc_plan(n, log2_group, log2_share)
    want = [[0] * n_public for _ in range(groups)]
    t0 = [0] * groups
    for i in range(n):
        g = group_of(i, half)
        t0[g] = (t0[g] + rs[i]) % R
        for j in range(n_public):
            want[g][j] = (want[g][j] + rs[i] * xs[i][j]) % R
    gi = groups // 2
    got, L = pkg.dbg_rlc_wide_group(b"".join(kpts), alpha, weights, live, inputs, n_public, n, log2_group, log2_share, gi)
    assert len(got) == groups
    assert [[int.from_bytes(s, "big") for s in row] for row in got] == want
    exp = O.g1_mul(kpts[0], t0[gi])
    for j in range(n_public):
        exp = O.g1_add(exp, O.g1_mul(kpts[j + 1], want[gi][j]))
    assert L == exp


def test_dead_group_contributes_nothing(pkg, O):
    """A group whose proofs all failed (loader error, r-torsion, a dead lane): weight 0 everywhere, scalars 0, L the identity."""
    rng = random.Random(77)
    n_public, n = 12, 40
    weights, _, _, _, inputs = _case(rng, n_public, n, 0)
    kpts, alpha = _key(O, rng, n_public)
    half, groups = rlc_plan(n, 3)
    live = bytes(0 if group_of(i, half) == 2 else 1 for i in range(n))
    got, L = pkg.dbg_rlc_wide_group(b"".join(kpts), alpha, weights, live, inputs, n_public, n, 3, 0, 2)
    assert all(s == bytes(32) for s in got[2])
    assert any(s != bytes(32) for s in got[1])
    assert L == bytes(64)


def _parts(m, n_streams):
    parts = n_streams if n_streams > 1 and m >= n_streams * 16384 else 1
    while (m + parts - 1) // parts > G16_MAX_LAUNCH:
        parts += 1
    per = ((m + parts - 1) // parts + 255) // 256 * 256
    return [(lo, min(lo + per, m)) for lo in range(0, parts * per, per) if lo < m]


def _share(part_n, lg, ls, min_lanes):
    ls = min(ls, lg)
    while ls > 0 and (part_n >> ls) < max(1, min_lanes):
        ls -= 1
    return ls


def test_wide_buffers_hold_every_part(pkg):
    """Every launch part's groups lie inside what the context allocates for the chunk -- rows, digits and partial sums -- side by side, in order, and match the
    fold plan of its proofs."""
    sizes = [1, 63, 64, 255, 257, 4096, 4097, 16383, 32768, 32769, 65536, 100001, 262144, 786433, 1 << 20]
    for key_inputs, form in ((9, 2), (16, 2), (17, 0), (40, 0), (40, 1), (1024, 0)):
        chunks = (key_inputs + 15) // 16
        for m in sizes:
            for n_streams, lg, ls, min_lanes in ((1, 5, 3, 65536), (2, 5, 3, 65536), (2, 1, 0, 1), (4, 8, 3, 1), (2, 16, 3, 1024)):
                alloc, parts = pkg.dbg_rlc_wide_plan(m, n_streams, lg, ls, min_lanes, key_inputs, form)
                want = _parts(m, n_streams)
                assert len(parts) == len(want)
                off = 0
                for (first, groups), (lo, hi) in zip(parts, want):
                    assert first == off
                    assert groups == rlc_plan(hi - lo, lg, _share(hi - lo, lg, ls, min_lanes))[1]
                    off += groups
                assert off * key_inputs * 32 <= alloc["rows"]
                assert alloc["digits"] == (off + 255) // 256 * 256 * 20 * key_inputs * 2 if form == 0 else alloc["digits"] == 0
                assert off * chunks * 27 * 4 <= alloc["part"] if form != 2 else alloc["part"] == 0


def test_status_regions_of_the_parts(pkg):
    """The group status bytes of the same parts, over the same grid: part k's region starts at the sum of round256(groups) of the parts before it (the probe hands
    out the groups; the offsets are derived from them here), every region lies inside what the context allocates for the chunk, and the last one ends at what
    bn254_dbg_g16_rlc_plan reports as the chunk's need."""
    import ctypes as C
    L = pkg.lib()
    L.bn254_dbg_g16_rlc_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    need, held = C.c_uint64(), C.c_uint64()
    sizes = [1, 63, 64, 255, 257, 4096, 4097, 16383, 32768, 32769, 65536, 100001, 262144, 786433, 1 << 20]
    for m in sizes:
        for n_streams, lg, ls, min_lanes in ((1, 5, 3, 65536), (2, 5, 3, 65536), (2, 1, 0, 1), (4, 8, 3, 1), (2, 16, 3, 1024)):
            _, parts = pkg.dbg_rlc_wide_plan(m, n_streams, lg, ls, min_lanes, 9, 2)
            assert L.bn254_dbg_g16_rlc_plan(m, m, n_streams, lg, ls, min_lanes, C.byref(need), C.byref(held)) == 0
            want = _parts(m, n_streams)
            assert len(parts) == len(want)
            grp_off = 0
            for (_, groups), (lo, hi) in zip(parts, want):
                assert groups == rlc_plan(hi - lo, lg, _share(hi - lo, lg, ls, min_lanes))[1]
                grp_off += (groups + 255) // 256 * 256
                assert grp_off <= held.value, (m, n_streams, lg, ls, min_lanes)
            assert grp_off == need.value, (m, n_streams, lg, ls, min_lanes)
