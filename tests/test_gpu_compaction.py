"""Compaction of the lane launches of the exact Groth16 path (csrc/bn254_g16_plan.h::g16_compacts): k_g16_classify decides the proofs the loader
rejects for good, k_g16_compact_write lists the rest, and k_g16_prepare and every kernel after it run on that dense list.

Every case compares EVERY status byte with the CPU oracle (groth16_verify_many, MODE_REFERENCE), runs the same call twice and requires identical bytes, and starts from
a status buffer filled with 0xEE: no 0xEE and no 0x80 (the internal "pending") may survive.  The oracle takes milliseconds per proof, so a batch is laid out from a
small pool of DISTINCT records -- proofs of synth_groth16 (valid ones, and its five failure classes) and byte mutations of them made here -- whose statuses the oracle
computes once; which record sits in which lane is what compaction is sensitive to, and that is what the cases vary.

Sizes: 30 800, just above the hand-over from the cooperative kernels (30 720), not a multiple of 256 -- the smallest batch the plan sends down the lane path -- and
65 552, two sub-batches side by side (33 024 + 32 528 proofs with two streams), the second ragged."""
import pytest

N_PUBLIC = 2
SEED = 0xC0A7C0DE
N_SMALL, N_TWO = 30800, 65552
FF = b"\xff" * 32


@pytest.fixture(scope="module")
def env(pkg, O):
    """the key, the pool of distinct (record, input row) pairs by kind, the oracle's status of each (computed once), and the prepared key"""
    vk, good_p, good_i, good_e = pkg.synth_groth16(SEED, N_PUBLIC, 24, invalid_every=0, agree=True, threads=8)
    vk2, bad_p, bad_i, bad_e = pkg.synth_groth16(SEED, N_PUBLIC, 40, invalid_every=1, agree=True, threads=8)
    assert vk == vk2 and set(good_e) == {pkg.ACCEPT}
    row = 32 * N_PUBLIC
    good = [(good_p[256 * i:256 * i + 256], good_i[row * i:row * i + row]) for i in range(24)]
    bad = [(bad_p[256 * i:256 * i + 256], bad_i[row * i:row * i + row]) for i in range(40)]      # class i % 5: input, pairing, A off the curve, B outside G2, range
    cache = {}

    def oracle(rec):
        if rec not in cache:
            cache[rec] = O.groth16_verify_many(rec[0], 256, vk, rec[1], N_PUBLIC, 1, O.MODE_REFERENCE)[0]
        return cache[rec]

    for i, rec in enumerate(bad):
        assert oracle(rec) == bad_e[i]
    # what the loader decides for good (k_g16_classify): classes 2 and 4 of the generator
    assert {oracle(r) for r in bad[2::5]} == {pkg.ERR_NOT_ON_CURVE} and {oracle(r) for r in bad[4::5]} == {pkg.ERR_NOT_MEMBER}
    assert {oracle(r) for r in bad[3::5]} == {pkg.ERR_NOT_IN_SUBGROUP} and {oracle(r) for r in bad[0::5] + bad[1::5]} == {pkg.REJECT}
    pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
    yield {"pkg": pkg, "vk": vk, "good": good, "bad": bad, "oracle": oracle, "pvk": pvk}
    pvk.close()


def _run(env, recs):
    """the batch through the device entry, twice, from a status buffer of 0xEE; every byte against the oracle"""
    import torch
    pkg, pvk, n = env["pkg"], env["pvk"], len(recs)
    dev = torch.device("cuda:0")
    d_proofs = torch.frombuffer(bytearray(b"".join(r[0] for r in recs)), dtype=torch.uint8).to(dev)
    d_inputs = torch.frombuffer(bytearray(b"".join(r[1] for r in recs)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.current_stream(dev)
    runs = []
    for _ in range(2):
        d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        pvk.verify_batch_device(d_proofs.data_ptr(), d_inputs.data_ptr(), d_status.data_ptr(), n, 256, N_PUBLIC, 0, stream.cuda_stream)
        stream.synchronize()
        runs.append(bytes(d_status.cpu().numpy().tobytes()))
    got = runs[0]
    assert 0xEE not in got and 0x80 not in got, (got.count(0xEE), got.count(0x80))
    assert runs[1] == got, "the same call twice gave different bytes"
    want = bytes(env["oracle"](r) for r in recs)
    diff = [i for i in range(n) if got[i] != want[i]]
    assert not diff, (len(diff), [(i, got[i], want[i]) for i in diff[:10]])
    return got


def _with(rec, **fields):
    """a copy of the record with 32-byte fields replaced: ax ay | bx1 bx0 by1 by0 | cx cy"""
    off = {"ax": 0, "ay": 32, "bx1": 64, "bx0": 96, "by1": 128, "by0": 160, "cx": 192, "cy": 224}
    p = bytearray(rec[0])
    for k, v in fields.items():
        p[off[k]:off[k] + 32] = v
    return bytes(p), rec[1]


def _plus_one(field):
    return (int.from_bytes(field, "big") + 1).to_bytes(32, "big")


def _layout(env, n, invalid_every):
    """the generator's pattern from the pool: proof i is invalid when i % invalid_every == invalid_every - 1, its class (i // invalid_every) % 5"""
    good, bad = env["good"], env["bad"]
    if invalid_every == 0:
        return [good[i % len(good)] for i in range(n)]
    return [bad[(i // invalid_every) % len(bad)] if i % invalid_every == invalid_every - 1 else good[i % len(good)] for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,invalid_every", [(N_SMALL, 16), (N_SMALL, 1), (N_SMALL, 0), (N_TWO, 16), (N_TWO, 1)])
def test_generator_pattern(env, n, invalid_every):
    """1/16 invalid (the benchmark's share: one decided proof per 40, never a whole wavefront), every proof invalid with the five classes cycling (2/5 decided by the
    loader), and nothing invalid (n' = n: the list is the batch)"""
    pkg = env["pkg"]
    got = _run(env, _layout(env, n, invalid_every))
    if invalid_every == 0:
        assert set(got) == {pkg.ACCEPT}
    else:
        assert set(got) >= {pkg.REJECT, pkg.ERR_NOT_IN_SUBGROUP, pkg.ERR_NOT_ON_CURVE, pkg.ERR_NOT_MEMBER}
        k = n // invalid_every
        assert abs(got.count(pkg.ERR_NOT_ON_CURVE) + got.count(pkg.ERR_NOT_MEMBER) - 2 * k // 5) <= 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_SMALL, N_TWO])
def test_every_proof_decided_by_the_loader(env, n):
    """A.x = 0xff.. everywhere: n' = 0, every wavefront after k_g16_compact_write leaves in its prologue"""
    recs = [_with(r, ax=FF) for r in env["good"]]
    got = _run(env, [recs[i % len(recs)] for i in range(n)])
    assert set(got) == {env["pkg"].ERR_NOT_MEMBER}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_SMALL, N_TWO])
def test_decided_proofs_at_the_edges_of_blocks(env, n):
    """decided proofs in the first lane of a block of 256, in the last lane of one, over a whole wavefront, over a whole block and over the last, partial block of the
    batch (and, at two sub-batches, the same around the cut between them)"""
    pkg, good, bad = env["pkg"], env["good"], env["bad"]
    decided = [bad[2], bad[4], bad[7], bad[9], _with(good[0], ax=FF), _with(good[1], by0=_plus_one(good[1][0][160:192]))]
    assert {env["oracle"](r) for r in decided} == {pkg.ERR_NOT_ON_CURVE, pkg.ERR_NOT_MEMBER}
    where = {3 * 256, 5 * 256 + 255} | set(range(7 * 256 + 64, 7 * 256 + 128)) | set(range(9 * 256, 10 * 256)) | set(range(n // 256 * 256, n))
    assert n % 256 != 0
    if n == N_TWO:
        for cut in (32768, 33024):                    # 33 024: where the first sub-batch ends with two streams (bn254_g16_plan.h::g16_plan_chunk); 32 768: half the batch
            where |= {cut - 1, cut, cut + 255} | set(range(cut + 512, cut + 576))
    recs = [decided[i % len(decided)] if i in where else good[i % len(good)] for i in range(n)]
    got = _run(env, recs)
    assert all((got[i] == pkg.ACCEPT) == (i not in where) for i in range(n))


@pytest.mark.gpu
def test_error_precedence(env):
    """the reference's order -- A, then B (member, curve), then B's subgroup, then C -- through the compaction: an error of C is NOT final for the loader (B outside G2
    ranks ahead of it), an error of A or B is"""
    pkg, good, bad, oracle = env["pkg"], env["good"], env["bad"], env["oracle"]
    g = good[2]
    out_b = bad[3][0][64:192]                         # a twist point outside G2 (class 3 of the generator)
    b_fields = dict(bx1=out_b[0:32], bx0=out_b[32:64], by1=out_b[64:96], by0=out_b[96:128])
    c_off, c_big = dict(cy=_plus_one(g[0][224:256])), dict(cx=FF)
    a_off, a_big = dict(ay=_plus_one(g[0][32:64])), dict(ax=FF)
    by_off, bx_big = dict(by0=_plus_one(g[0][160:192])), dict(bx1=FF)
    cases = [
        (_with(g, **c_off, **b_fields), pkg.ERR_NOT_IN_SUBGROUP), (_with(g, **c_big, **b_fields), pkg.ERR_NOT_IN_SUBGROUP),     # bad C, B outside G2: the subgroup error
        (_with(g, **c_off), pkg.ERR_NOT_ON_CURVE), (_with(g, **c_big), pkg.ERR_NOT_MEMBER),                                     # bad C, good B: C's error
        (_with(g, **a_big, **by_off), pkg.ERR_NOT_MEMBER), (_with(g, **a_off, **bx_big), pkg.ERR_NOT_ON_CURVE),                 # bad A, bad B: A's error
        (_with(g, **by_off, **c_big), pkg.ERR_NOT_ON_CURVE), (_with(g, **bx_big, **c_off), pkg.ERR_NOT_MEMBER),                 # bad B, bad C: B's error
        (_with(g, **a_off, **b_fields, **c_big), pkg.ERR_NOT_ON_CURVE),
    ]
    for rec, want in cases:
        assert oracle(rec) == want, (oracle(rec), want)
    n = N_SMALL
    recs = [good[i % len(good)] for i in range(n)]
    for k in range(0, n, 37):                         # 37: every lane position of a wavefront and of a block gets every case
        recs[k] = cases[(k // 37) % len(cases)][0]
    got = _run(env, recs)
    for k in range(0, n, 37):
        assert got[k] == cases[(k // 37) % len(cases)][1]
