"""Raw-digit operands of the value-level probes (bn254_dbg_coop12_op, bn254_dbg_fp12_op_fmt, bn254_dbg_verdict with in_format = 1).

csrc/bn254_fp.h keeps an Fp number as nine signed 32-bit words holding balanced 29-bit digits of ANY representative of its Montgomery residue
m = x * 2^261 mod p: value = sum d_i 2^(29 i), the eight low digits in [-2^28, 2^28), the top digit whatever is left.  Nothing but fp_canon resolves the
representative, so a test that wants to know what the kernels make of m + p, m - p or of a residue with a hostile digit pattern has to write the digits itself.
Pure Python integers; no part of the product is involved."""
import struct

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
NL, LB = 9, 29
HALF = 1 << (LB - 1)
MASK = (1 << LB) - 1
R261 = pow(2, NL * LB, P)
R261_INV = pow(R261, -1, P)
# what the operations accept: normalised low digits and |value| <= 2 p
CONTRACT_VB = 2


def mont(x):
    """The Montgomery residue of the field value x, in [0, p)."""
    return x % P * R261 % P


def encode(v):
    """The integer v (any sign) as nine balanced digits: the eight low ones in [-2^28, 2^28), the top one takes the rest."""
    d = []
    for _ in range(NL - 1):
        r = ((v + HALF) & MASK) - HALF
        d.append(r)
        v = (v - r) >> LB
    if not -(1 << 31) <= v < (1 << 31):
        raise ValueError("value does not fit nine digits")
    d.append(v)
    return d


def decode(d):
    """The integer nine digits stand for."""
    return sum(int(x) << (LB * i) for i, x in enumerate(d))


def field_value(d):
    """The field value in [0, p) of a Montgomery representative given by its digits."""
    return decode(d) * R261_INV % P


def in_contract(d, vb=CONTRACT_VB, negated=False):
    """The input contract of the Fp12 operations: eight low digits balanced, |value| <= vb * p.  negated: a digit of +2^28 passes too -- what the kernels' own
    digit-wise negation makes of -2^28 (bn254_fp.h::fp_neg; the bound tracker's lb = 0.5 is |digit| <= 2^28)."""
    return len(d) == NL and all(-HALF <= x < HALF + (1 if negated else 0) for x in d[:NL - 1]) and abs(decode(d)) <= vb * P


def pattern(kind, top):
    """A residue picked for its digits: the eight low digits all -2^28 (kind 0), all 2^28 - 1 (1) or alternating (2: -2^28 first; 3: 2^28 - 1 first), top digit
    `top`.  These are the extremes of every column sum of a digit product."""
    lo, hi = -HALF, HALF - 1
    low = {0: [lo] * 8, 1: [hi] * 8, 2: [lo, hi] * 4, 3: [hi, lo] * 4}[kind]
    return low + [top]


def pack12(reps):
    """Twelve digit lists (tower order) -> the 432 bytes of one Fp12 operand in format 1."""
    assert len(reps) == 12
    return b"".join(struct.pack("<9i", *d) for d in reps)


def unpack12(b):
    """432 bytes in format 1 -> twelve digit lists."""
    w = struct.unpack("<108i", b)
    return [list(w[NL * t:NL * t + NL]) for t in range(12)]


def bytes12(vals):
    """Twelve field values (tower order) -> the 384 bytes of format 0."""
    return b"".join(int(v % P).to_bytes(32, "big") for v in vals)


def vals12(b):
    return [int.from_bytes(b[32 * t:32 * t + 32], "big") for t in range(12)]
