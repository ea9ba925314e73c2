"""The PlonK stage kernels (k_plonk_stage1, k_plonk_stage2 and their _keys twins, csrc/bn254_k_plonk.hip) held to the oracle BY VALUE, proof by proof.

bn254_dbg_plonk_stages runs the product's own pass up to the pairing operands under a ChaCha20 key the test gives and returns, per proof: the stage-1 status, zeta,
lambda, the opening of the linearised polynomial, every BSB22 hash-to-field value, the digest the first MSM produced, the status after stage 2, and P0 / P1 as the
second MSM stored them.  The expectation (tests/plonk_stage_ref.py) comes from oracle calls, hashlib and the ChaCha20 block function alone;
tests/test_plonk_stage_values_cpu.py has proven it against the host compile of the stages where there is no GPU.  Every comparison is byte equality.  The digest of
the linearised polynomial, which no oracle call gives, must be a curve point and equal the host compile's."""

import pytest

import plonk_stage_ref as ref
from kzg_forgery import forge
from plonk_keys_common import Batch, diff, shuffled

pytestmark = pytest.mark.gpu

SHAPES = [(0, 0, 3), (1, 0, 4), (2, 1, 12), (9, 1, 5), (40, 2, 7), (8, 8, 6)]      # (n_public, n_qcp, log2 rows)
KEY = [0x9e3779b9, 0x7f4a7c15, 0xf39cc060, 0x5cedc834, 0x1082276b, 0xf3a27251, 0xf86c6a11, 0xd0c18e95, 0x2767f0b1, 0x53d8b4f0, 0x0c4f1a3d]
N = 67                    # one workgroup plus three lanes
N_EDGE = 130              # two workgroups plus two lanes
EDGE = (2, 1, 12)
PAIRING_FAILED = 8


def _classes(shape):
    """the statuses bn254_synth_plonk gives a shape at invalid_every = 3 (the oracle confirms each below)"""
    return {1, 2, 3, 8} | ({7} if shape[0] else set()) | ({9} if shape[1] else set())


class _Key:
    """a key shape with n generated proofs, every third invalid, and -- computed once, on demand, never changed -- the oracle's expectation of every proof under KEY
    with the proof's own index as its slot"""

    def __init__(self, pkg, shape, n):
        self.shape, self.n, self.n_public, self.n_qcp, self.plen = shape, n, shape[0], shape[1], 808 + 96 * shape[1]
        seed = 0x57A6E000 + 4096 * shape[0] + 64 * shape[1] + shape[2]          # its own seed: its own SRS
        self.vk, self.proofs, self.inputs, self.exp = pkg.synth_plonk(seed, shape[0], shape[1], shape[2], n, invalid_every=3, threads=16)
        self.pvk = pkg.PreparedPlonkVk(self.vk)
        self._want, self._host = [], None

    def proof(self, j):
        return self.proofs[self.plen * j:self.plen * (j + 1)]

    def row(self, j):
        return self.inputs[32 * self.n_public * j:32 * self.n_public * (j + 1)]

    def rows(self, j):
        return ref.rows(self.inputs, self.n_public, j)

    def want(self, O, n=N):
        """the expectations of the first n proofs (three oracle calls each, made once)"""
        while len(self._want) < n:
            i = len(self._want)
            self._want.append(ref.expect(O, self.vk, self.proof(i), self.rows(i), self.n_qcp, ref.lam_of(KEY, i), slot=i))
            assert self._want[i]["oracle_status"] == self.exp[i]                      # the generator's statuses, confirmed by the oracle
        assert set(self.exp[:n]) == _classes(self.shape) and sum(w["status1"] == ref.ACCEPT for w in self._want[:n]) >= 40
        return self._want

    def host(self, pkg):
        """the host compile's records under KEY (for the digest of the linearised polynomial)"""
        if self._host is None:
            self._host = pkg.dbg_plonk_stages(self.pvk, self.proofs, self.inputs, KEY, n=self.n, proof_stride=self.plen, device=-1)
        return self._host

    def strided(self, stride, n):
        return b"".join(self.proof(i) + b"\xa5" * (stride - self.plen) for i in range(n))


@pytest.fixture(scope="module")
def torch_dev(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the product has no CPU fallback"
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def keys(pkg, torch_dev):
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = _Key(pkg, shape, N_EDGE)
        return cache[shape]

    yield get
    for k in cache.values():
        k.pvk.close()


def _check(pkg, O, k, got, n, what):
    want = k.want(O, max(n, N))
    assert len(got) == n
    for i in range(n):
        ref.compare(got[i], want[i], "%s, proof %d of %d" % (what, i, n))
        assert got[i]["lin"] == k.host(pkg)[i]["lin"], "%s, proof %d: the digest of the linearised polynomial differs from the host compile's" % (what, i)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_every_shape_every_value(pkg, O, keys, shape):
    """67 proofs at the packed stride under one fixed non-zero key: every output of the probe against the oracle, proof by proof.  From 9 public inputs on the rows are
    not staged in LDS: (9,1,5) and (40,2,7) read them through lane_inputs in every workgroup of the batch"""
    k = keys(shape)
    got = pkg.dbg_plonk_stages(k.pvk, k.proofs[:k.plen * N], k.inputs[:32 * k.n_public * N], KEY, n=N, proof_stride=k.plen)
    _check(pkg, O, k, got, N, "shape %r" % (shape,))
    assert set(k.exp[:N]) == _classes(shape)
    assert sum(g["status1"] == ref.ACCEPT for g in got) >= 40 and sum(g["p0"] != ref.ZERO64 for g in got) >= 40          # not a pass on all-failures
    if shape != EDGE:
        return
    # rows that hold 0, 1 and r - 1, with proofs made for them
    vals = [0, 1, ref.R - 1]
    rows = b"".join(ref.be32(a) + ref.be32(b) for a in vals for b in vals)
    vk, proofs = pkg.synth_plonk_for_inputs(0x57A6E001, 2, 1, 12, rows, threads=16)
    pvk = pkg.PreparedPlonkVk(vk)
    try:
        got = pkg.dbg_plonk_stages(pvk, proofs, rows, KEY, n=9, proof_stride=904)
        host = pkg.dbg_plonk_stages(pvk, proofs, rows, KEY, n=9, proof_stride=904, device=-1)
        for i in range(9):
            want = ref.expect(O, vk, proofs[904 * i:904 * (i + 1)], ref.rows(rows, 2, i), 1, ref.lam_of(KEY, i), slot=i)
            assert want["oracle_status"] == ref.ACCEPT
            ref.compare(got[i], want, "edge inputs, proof %d" % i)
            assert got[i]["lin"] == host[i]["lin"]
    finally:
        pvk.close()


def test_batch_and_stride_edges(pkg, O, keys):
    """pl_stage_rows moves sixteen records per step behind rec < n guards, and takes the dword path only when both base pointers and both strides are multiples of 4:
    tails of 1, 15, 16 and 17 lanes, one and two workgroups and a workgroup plus one, at the packed stride 904, at 905 (the byte path) and 908, at the most the
    parser reads (1664 = PL_STAGE_MAX_PROOF) and beyond it (1700), 0xA5 behind every proof.  Every run equals the prefix of ONE expectation of 130 proofs: the values
    of proof i depend on neither n nor the stride"""
    k = keys(EDGE)
    k.want(O, N_EDGE)
    for stride in (904, 905, 908, 1664, 1700):
        recs = k.strided(stride, N_EDGE)
        for n in (1, 15, 16, 17, 63, 64, 65, 130):
            got = pkg.dbg_plonk_stages(k.pvk, recs[:stride * n], k.inputs[:64 * n], KEY, n=n, proof_stride=stride)
            _check(pkg, O, k, got, n, "stride %d, n %d" % (stride, n))


def test_largest_lds_request(pkg, O, keys):
    """8 public inputs are the widest row that is staged and 1664 bytes the most of a record: by pl_lane_stride a lane then has 64 (SHA block) + 1664 + 256 = 1984 bytes =
    496 dwords, made odd: 497 dwords = 1988 bytes, and k_plonk_stage1 asks for 16 + 64 x 1988 + 64 x 68 (the helper lanes' SHA blocks, PL_HELPER_SHA_STRIDE) =
    131 600 bytes of dynamic LDS -- the largest request the launcher can make (derived, not measured).  The values are those at the packed stride"""
    k = keys((8, 8, 6))
    assert k.plen == 1576
    got = pkg.dbg_plonk_stages(k.pvk, k.strided(1700, 65), k.inputs[:256 * 65], KEY, n=65, proof_stride=1700)
    _check(pkg, O, k, got, 65, "stride 1700, 8 inputs")
    assert got == pkg.dbg_plonk_stages(k.pvk, k.proofs[:k.plen * 65], k.inputs[:256 * 65], KEY, n=65, proof_stride=k.plen)
    assert sum(g["status1"] == ref.ACCEPT for g in got) >= 40


def test_lambda_stream(pkg, O, keys, fixtures):
    """lambda_i = blocks 3i .. 3i + 2 of the call's stream, per proof: a kernel that gave every lane lane 0's, dropped a block or ignored a nonce word fails here.  Then
    the forgery of kzg_forgery.py against lambda_37 of the key: it verifies in slot 37 and nowhere else, and the public entry, which draws its own key, rejects it"""
    k = keys(EDGE)
    other = list(KEY); other[9] ^= 1 << 17
    args = (k.pvk, k.proofs[:k.plen * N], k.inputs[:64 * N])
    a = pkg.dbg_plonk_stages(*args, KEY, n=N, proof_stride=k.plen)
    b = pkg.dbg_plonk_stages(*args, other, n=N, proof_stride=k.plen)
    live = [i for i in range(N) if a[i]["status1"] == ref.ACCEPT]
    assert len(live) >= 40 and [i for i in range(N) if b[i]["status1"] == ref.ACCEPT] == live
    assert all(a[i]["lambda"] != b[i]["lambda"] for i in live)                                              # one nonce bit moves every lambda
    assert len({a[i]["lambda"] for i in live}) == len(live)                                                 # pairwise distinct
    assert all(a[i]["lambda"] == ref.be32(ref.lam_of(KEY, i)) and b[i]["lambda"] == ref.be32(ref.lam_of(other, i)) for i in live)
    assert all(a[i]["p0"] != b[i]["p0"] and a[i]["p1"] != b[i]["p1"] and a[i]["zeta"] == b[i]["zeta"] for i in live)
    # the forged proof on the reference's key (2 inputs, 1 commitment)
    fx, vk = fixtures
    f = fx["fibonacci_plonk"]
    proof, pis = bytes.fromhex(f["raw_proof"]), [int(x) for x in f["public_inputs"]]
    row = b"".join(ref.be32(x) for x in pis)
    lam37 = ref.lam_of(KEY, 37)
    tampered, forged = forge(O, proof, vk, pis, lam37)
    pvk = pkg.PreparedPlonkVk(vk)
    try:
        for at in (37, 36):
            lam = ref.lam_of(KEY, at)
            batch = b"".join(forged if i == at else proof for i in range(N))
            got = pkg.dbg_plonk_stages(pvk, batch, row * N, KEY, n=N, proof_stride=904)
            verdict = O.plonk_verify(forged, vk, pis, lam=lam)
            assert verdict == (ref.ACCEPT if at == 37 else PAIRING_FAILED)
            st, (p0, p1), _ = O.plonk_pairing_inputs_lam(forged, vk, pis, lam)
            assert st == verdict and got[at]["status"] == ref.ACCEPT and (got[at]["p0"], got[at]["p1"]) == (p0, p1) and got[at]["lambda"] == ref.be32(lam)
            if at == 36:      # ... and they are NOT the points the forger aimed at
                assert got[at]["p0"] != O.plonk_pairing_inputs_lam(forged, vk, pis, lam37)[1][0]
            honest = ref.expect(O, vk, proof, [ref.be32(x) for x in pis], 1, ref.lam_of(KEY, 5), slot=5)
            ref.compare(got[5], honest, "honest fixture proof in slot 5")
            status = pvk.verify_batch(batch, row * N, n=N, proof_stride=904)
            assert status == bytes(PAIRING_FAILED if i == at else ref.ACCEPT for i in range(N))
    finally:
        pvk.close()


def test_weights(pkg, O, keys):
    """BN254_FLAG_RLC: P0' = w_i P0 and P1' = w_i P1 with w_i from the second stream (nonce word 2 xor "RLC"), 128 bits, forced odd.  A weight stream equal to the
    lambda stream, or one that ignored the slot, fails here"""
    k = keys(EDGE)
    want = k.want(O, N)
    got = pkg.dbg_plonk_stages(k.pvk, k.proofs[:k.plen * N], k.inputs[:64 * N], KEY, n=N, proof_stride=k.plen, flags=pkg.FLAG_RLC)
    ws = [ref.weight_of(KEY, i) for i in range(N)]
    assert all(w & 1 and w < 1 << 128 for w in ws) and len(set(ws)) == N
    lam_words = {ref.lam_of(KEY, i) for i in range(N)} | {int.from_bytes(ref.be32(ref.lam_of(KEY, i))[16:], "big") for i in range(N)}
    unweighted = [ref.weight_of([w for w in KEY[:10]] + [KEY[10] ^ ref.RLC_NONCE_TWIST], i) for i in range(N)]          # the same words drawn from the lambda stream
    assert not set(ws) & lam_words and not set(ws) & set(unweighted)
    live = 0
    for i in range(N):
        w = want[i]
        if w["status1"] == ref.ACCEPT:
            live += 1
            assert not w.get("ambiguous")
            w = dict(w, p0=O.g1_mul(w["p0"], ws[i]), p1=O.g1_mul(w["p1"], ws[i]))
            assert got[i]["p0"] != O.g1_mul(want[i]["p0"], unweighted[i])
        ref.compare(got[i], w, "weighted, proof %d" % i)
        assert got[i]["lin"] == k.host(pkg)[i]["lin"]
    assert live >= 40


LISTS = [[(2, 1, 12), (9, 1, 5), (1, 1, 4)],      # a staged key beside a member that reads its rows from memory
         [(40, 1, 7), (9, 1, 5)],                 # nothing staged
         [(8, 1, 5), (9, 1, 5)]]                  # at the staging boundary: the widest staged row beside the narrowest unstaged one


@pytest.mark.parametrize("shapes", LISTS, ids=lambda l: "+".join("%d-%d-%d" % s for s in l))
def test_key_lists(pkg, O, keys, shapes):
    """130 shuffled proofs over a list whose members share one commitment: k_plonk_stage1_keys takes the key, the input count and whether the rows are staged per
    granule.  Every proof's values under the lambda OF ITS SLOT (the probe reports the slot; lambda and the weight are drawn per slot, not per proof), and the statuses
    of the public entry on the same buffers"""
    members = [keys(s) for s in shapes]
    counts = [N_EDGE // len(members) + (1 if p < N_EDGE % len(members) else 0) for p in range(len(members))]
    b = Batch(members, shuffled(counts, seed=len(shapes) + shapes[0][0]))
    assert b.n == N_EDGE and b.plen == 904
    ks = b.key_set(pkg)
    got = pkg.dbg_plonk_stages_keys(ks, b.index, b.proofs, b.rows, KEY, proof_stride=904, input_stride=b.input_stride)
    slots = [g["slot"] for g in got]
    assert len(set(slots)) == b.n and max(slots) < b.slots()
    granule_key = {}
    for g, p in zip(got, b.index):
        assert granule_key.setdefault(g["slot"] // 64, p) == p                      # a granule of 64 slots has one key
    live = 0
    for i, (p, j) in enumerate(b.items):
        m = members[p]
        want = ref.expect(O, m.vk, m.proof(j), m.rows(j), 1, ref.lam_of(KEY, slots[i]), slot=slots[i])
        assert want["oracle_status"] == m.exp[j]
        ref.compare(got[i], want, "list %r, proof %d (member %d, its proof %d, slot %d)" % (shapes, i, p, j, slots[i]))
        live += want["status1"] == ref.ACCEPT
    assert live >= 80
    status = b.host(ks)
    assert status == b.exp, diff(status, b.exp)


@pytest.mark.parametrize("shape", [EDGE, (9, 1, 5)], ids=lambda s: "%d-%d-%d" % s)
def test_unaligned_device_pointers(pkg, torch_dev, keys, shape):
    """the dword path of the staging loop also looks at the two base pointers: a proof tensor sliced from byte 1 and an input tensor sliced from byte 2, at the
    packed stride and at 905.  The statuses are the generator's"""
    torch, dev = torch_dev
    k = keys(shape)
    n = N_EDGE
    for stride in (904, 905):
        recs = k.strided(stride, n)
        d_p = torch.frombuffer(bytearray(b"\x5a" + recs), dtype=torch.uint8).to(dev)[1:]
        d_i = torch.frombuffer(bytearray(b"\x5a\x5a" + k.inputs[:32 * k.n_public * n]), dtype=torch.uint8).to(dev)[2:]
        assert d_p.data_ptr() % 4 == 1 and d_i.data_ptr() % 4 == 2
        d_s = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        k.pvk.verify_batch_device(d_p.data_ptr(), d_i.data_ptr(), d_s.data_ptr(), n, proof_stride=stride, n_public=k.n_public, device=dev.index,
                                  stream=torch.cuda.current_stream(dev).cuda_stream)
        got = bytes(d_s.cpu().numpy().tobytes())
        assert got == k.exp[:n], "stride %d: %s" % (stride, diff(got, k.exp[:n]))
    assert k.exp[:n].count(bytes([ref.ACCEPT])) >= 40
