"""Pairs of invalid proofs whose errors cancel under EQUAL batching weights: what BN254_FLAG_RLC must reject and an RLC pass with dependent weights accepts.

An RLC group passes when  sum_i r_i E_i = 0  for the per-proof errors E_i; with independent 128-bit weights that means every E_i = 0.  A pair with E_a = -E_b
passes whenever r_a = r_b -- the same ChaCha20 block for two lanes, for two proofs of a shared-accumulator lane or for both partners of a fold round, or weights
paired with the wrong member consistently across a group.  Neither forgery needs a trapdoor: only the oracle's group operations and Python integers.

Groth16, family C:   C_a + k T, C_b - T for a random T: the error sits in e(C, -delta), r_a k T - r_b T, zero exactly when r_b = k r_a.
Groth16, family X_j: x_{a,j} + d, x_{b,j} - d (mod r, canonical): the error is +-d K_{j+1} in L, zero exactly when the weights that reach t_j / s_j are equal.
PlonK:               the SAME valid proof twice, H + D and H - D (H is bound by no transcript: same zeta); the errors are (+zeta D, -D) and (-zeta D, +D) in
                     (P0, P1), whatever lambda each copy draws."""
from kzg_forgery import OFF_H

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GT_ONE = (1).to_bytes(32, "big") + bytes(352)
OFF_C = 192                      # a raw Groth16 record: A (64) | B (128) | C (64)


def be(v):
    return int(v).to_bytes(32, "big")


def g1_neg(p):
    return p if p == bytes(64) else p[:32] + be((P - int.from_bytes(p[32:64], "big")) % P)


def forge_c(O, proofs, a, b, T, k=1, stride=256):
    """In place: C_a += k T, C_b -= T (proofs: bytearray of raw records)."""
    for i, D in ((a, O.g1_mul(T, k % R)), (b, g1_neg(T))):
        o = stride * i + OFF_C
        proofs[o:o + 64] = O.g1_add(bytes(proofs[o:o + 64]), D)


def forge_x(inputs, n_public, a, b, j, d):
    """In place: x_{a,j} += d, x_{b,j} -= d modulo r, written canonically (inputs: bytearray of n_public x 32-byte rows)."""
    assert d % R
    for i, s in ((a, d), (b, -d)):
        o = 32 * (n_public * i + j)
        inputs[o:o + 32] = be((int.from_bytes(inputs[o:o + 32], "big") + s) % R)


def plonk_pair(O, proof, D):
    """The two copies of one valid PlonK proof with H + D and H - D."""
    h = proof[OFF_H:OFF_H + 64]
    return tuple(proof[:OFF_H] + O.g1_add(h, E) + proof[OFF_H + 64:] for E in (D, g1_neg(D)))


def x_positions(n_public, per_lane=16):
    """The inputs family X is planted at: first, last, one in the middle, and both sides of every boundary between the chunks of per_lane inputs a wide key's
    public-input sum runs in (G16_WIDE_MSM_INPUTS_PER_LANE)."""
    js = {0, n_public - 1, n_public // 2}
    for c in range(per_lane, n_public, per_lane):
        js |= {c - 1, c}
    return sorted(js)


# ---- the pair positions inside a group ----------------------------------------------------------------------------------------------------------------------------
def members_by_group(group):
    """group id -> its members, sorted (the slots of a group)."""
    out = {}
    for i, g in enumerate(group):
        out.setdefault(g, []).append(i)
    return out


def fold_halves(n, log2_group, log2_share):
    """bn254_rlc_plan.h::rlc_plan: the halves of the fold rounds of a launch part of n proofs."""
    m = (n + (1 << log2_share) - 1) >> log2_share
    half = [m << k for k in range(log2_share - 1, -1, -1)]
    target = max(1, n >> log2_group)
    cur = m
    while cur > target and len(half) < 28:
        cur = (cur + 1) // 2
        half.append(cur)
    return half, cur


def fold_group_of(i, half):
    """... ::rlc_group_of: i -= half[k] while i >= half[k], round by round."""
    for h in half:
        if i >= h:
            i -= h
    return i


def fold_bits(i, half):
    """The fold bits of proof i: bit k set when round k moved it (i = group + sum_k bit_k half[k])."""
    bits = 0
    for k, h in enumerate(half):
        if i >= h:
            i -= h
            bits |= 1 << k
    return bits


def fold_bit_pair(members, half, k, setting, rng):
    """Two members of one group that differ in fold bit k alone -- the partners of fold round k -- with the other bits all zero (setting 0), all one where such a
    member exists, else the largest setting that does (1), or drawn from rng (2).  None when the group has no such pair."""
    by_bits = {fold_bits(i, half): i for i in members}
    lows = sorted(b for b in by_bits if not (b >> k) & 1 and (b | 1 << k) in by_bits)
    if not lows:
        return None
    b = (lows[0], lows[-1], rng.choice(lows))[setting]
    return by_bits[b], by_bits[b | 1 << k]
