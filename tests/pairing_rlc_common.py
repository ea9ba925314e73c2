"""Batches for BN254_FLAG_RLC on the pairing batch (bn254_pairing_check_batch_flags, bn254_dbg_pairing_batch_rlc) for tests/test_pairing_rlc_cpu.py and
tests/test_gpu_pairing_rlc.py: layouts of the vectors of tests/pairing_shared_common.py over groups of 64 items, the probe's weights, and what the definition gives --
status bytes from the vectors, the GT value of every group from O.g1_mul and O.pairing.  Nothing here calls the library under test except g2_prepare for the records."""
import pairing_batch_common as V
import pairing_shared_common as S

SHAPES = ((1, 0b1), (2, 0b11), (2, 0b10), (4, 0b1110), (3, 0), (8, 0b10101010))
LAYOUTS = ("mixed", "one_reject", "decided_group")
PENDING = (V.ACCEPT, V.REJECT)

_PREP = {}


def prepared_of(pkg, O, k, mask):
    """the records of the shape's shared points, ascending position order (b"" without a shared position)"""
    if (k, mask) not in _PREP:
        shared, _ = S.vectors(O, k, mask)
        recs = []
        for j in sorted(shared):
            st, rec = pkg.g2_prepare(shared[j])
            assert st == V.ACCEPT
            recs.append(rec)
        _PREP[(k, mask)] = b"".join(recs)
    return _PREP[(k, mask)]


def _named(vecs, prefix):
    return [i for i, v in enumerate(vecs) if v[0].startswith(prefix)]


def layout(vecs, n, kind):
    """vector index of every item.  mixed: every vector class in every whole group; one_reject: valid items and ONE reject, alone in the middle group; decided_group: the
    first group (or the whole batch below 65 items) decided in phase 1, valid items behind it"""
    ok, bad = _named(vecs, "identity")[0], _named(vecs, "identity_perturbed")[0]
    assert vecs[ok][3] == V.ACCEPT and vecs[bad][3] == V.REJECT
    if kind == "mixed":
        return [i % len(vecs) for i in range(n)]
    if kind == "one_reject":
        groups = (n + 63) // 64
        g = groups // 2
        at = min(64 * g + 5, n - 1)
        return [bad if i == at else ok for i in range(n)]
    early = [i for i, v in enumerate(vecs) if v[3] in (V.NOT_MEMBER, V.NOT_ON_CURVE)]
    return [early[i % len(early)] if i < 64 else ok for i in range(n)]


def build(vecs, idx, k, mask):
    """(packed buffer, expected status bytes)"""
    return b"".join(vecs[j][1] for j in idx), bytes(vecs[j][3] for j in idx)


def weights_for(n, seed=0):
    """n distinct odd 128-bit weights, 16 big-endian bytes each"""
    return b"".join(((0x9E3779B97F4A7C15F39CC0605CEDC835 * (i + 1 + 1000 * seed)) % (1 << 128) | 1).to_bytes(16, "big") for i in range(n))


def weight_at(weights, i):
    return int.from_bytes(weights[16 * i:16 * i + 16], "big") | 1


def item_pairs(O, vec, k, r):
    """the (r P_j, Q_j) of an item that contribute to its product, from the EXPANDED item"""
    ps, qs = [], []
    for j in range(k):
        p, q = vec[2][192 * j:192 * j + 64], vec[2][192 * j + 64:192 * j + 192]
        if p == bytes(64) or q == bytes(128):
            continue
        ps.append(O.g1_mul(p, r % V.R)); qs.append(q)
    return ps, qs


def gt_of(O, ps, qs):
    return O.pairing(b"".join(ps), b"".join(qs)) if ps else V.GT_ONE


def expected_groups(O, vecs, idx, k, weights):
    """per group (GT bytes, status): the product over the group's pending items of prod_j e(r_i P_ij, Q_ij)"""
    out = []
    for g in range((len(idx) + 63) // 64):
        ps, qs = [], []
        for i in range(64 * g, min(64 * g + 64, len(idx))):
            if vecs[idx[i]][3] in PENDING:
                p, q = item_pairs(O, vecs[idx[i]], k, weight_at(weights, i))
                ps += p; qs += q
        gt = gt_of(O, ps, qs)
        out.append((gt, V.ACCEPT if gt == V.GT_ONE else V.REJECT))
    return out


def forgery(pkg, O, shared_first):
    """Two valid two-pair items a, b with the same G2 point at position 0 -- shared (shape (2, 0b11)) or variable with equal bytes (shape (2, 0b10)) -- and the cancelling
    pair made of them: P_a0 + T and P_b0 - T.  ((k, mask), prepared records, packed items of the honest pair, packed items of the forged pair)"""
    import random
    rng = random.Random(0xF0E6 + shared_first)
    g1, g2 = O.g1_gen(), O.g2_gen()
    b0, b1 = rng.randrange(1, V.R), rng.randrange(1, V.R)
    q0, q1 = O.g2_mul(g2, b0), O.g2_mul(g2, b1)
    mask = 0b11 if shared_first else 0b10
    recs = b"".join(pkg.g2_prepare(q)[1] for q in ((q0, q1) if shared_first else (q1,)))
    t = rng.randrange(1, V.R)

    def item(a0, shift):
        a1 = (V.R - a0 * b0 % V.R) * pow(b1, -1, V.R) % V.R      # a0 b0 + a1 b1 = 0 for the honest a0
        p0, p1 = O.g1_mul(g1, (a0 + shift) % V.R), O.g1_mul(g1, a1)
        return p0 + (b"" if shared_first else q0) + p1

    a0, c0 = rng.randrange(1, V.R), rng.randrange(1, V.R)
    return (2, mask), recs, item(a0, 0) + item(c0, 0), item(a0, t) + item(c0, V.R - t)
