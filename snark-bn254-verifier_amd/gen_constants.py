#!/usr/bin/env python3
"""Generates csrc/bn254_constants.h: every BN254 constant the device/host arithmetic needs, in the
9 x 29-bit-limb Montgomery representation (R = 2^261) used by bn254_fp.h.

All values are derived here from p, r, u alone with Python integers, so the header
holds no hand-typed magic numbers.  Run:  python gen_constants.py > csrc/bn254_constants.h
"""
import sys

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_ORD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
U = 4965661367192848881
NL, LB = 9, 29
MASK = (1 << LB) - 1
RBITS = NL * LB
MONT_R = 1 << RBITS

assert P == 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1
assert R_ORD == 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1


def limbs(v):
    """balanced digits: v = sum d_i 2^(29 i), d_i in [-2^28, 2^28) (top digit takes what is left)"""
    assert 0 <= v < (1 << (RBITS - 1))
    out = []
    for i in range(NL):
        d = v & MASK
        if d >= (1 << (LB - 1)) and i < NL - 1:
            d -= 1 << LB
        out.append(d)
        v = (v - d) >> LB
    assert v == 0
    assert sum(d << (LB * i) for i, d in enumerate(out)) >= 0
    return out


def mont(v):
    return (v % P) * MONT_R % P


def arr(v):
    return "{" + ", ".join("%d" % x for x in limbs(v)) + "}"


# ---- Fp2 helpers (for Frobenius constants) ----
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2mul(r, a)
        a = f2mul(a, a)
        e >>= 1
    return r


def f2inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, (-a[1]) * n % P)


XI = (9, 1)


def naf(n):
    out = []
    while n:
        if n & 1:
            d = 2 - (n & 3)
            n -= d
        else:
            d = 0
        out.append(d)
        n >>= 1
    return out


# ---- x^u as an addition-subtraction chain (found by tools/search_u_chain.py; the width-4 signed windows it replaces: 63 squarings + 16 products) ----
U_CHAIN_RUN_MAX = 7        # squarings of one f12_cyclo_sqr_n operation
U_CHAIN_TABLE_MAX = 3      # table slots of vm_exp_u besides x
U_CHAIN_TABLE = (5, 9, 19)
# operands: 0 = x, 1 = the temporary, 2 + i = table entry i.  (op, dst, a, b): op 0: dst <- a^(2^b), op 1: dst <- a * b
U_CHAIN_BUILD = ((0, 1, 0, 2),      # x^4
                 (1, 2, 1, 0),      # x^5 = x^4 x
                 (1, 3, 2, 1),      # x^9 = x^5 x^4
                 (0, 1, 2, 1),      # x^10 = (x^5)^2
                 (1, 4, 1, 3))      # x^19 = x^10 x^9
# MSB first: (digit, squarings before the next digit)
U_CHAIN_MAIN = ((19, 3), (-19, 2), (19, 6), (19, 7), (19, 6), (-19, 7), (9, 6), (19, 5), (9, 7), (5, 5), (-1, 4), (1, 0))


def u_chain():
    """The chain, checked in Python integers: it evaluates to u, the table has at most three entries besides x and each holds what the digits
    expect of it, no run exceeds the limit, and no step reads an operand before it is written or writes x."""
    assert len(U_CHAIN_TABLE) <= U_CHAIN_TABLE_MAX
    val = {0: 1}
    squarings = products = 0
    for op, dst, a, b in U_CHAIN_BUILD:
        assert op in (0, 1) and 1 <= dst < 2 + len(U_CHAIN_TABLE) and a in val
        if op == 0:
            assert 1 <= b <= U_CHAIN_RUN_MAX
            val[dst] = val[a] << b; squarings += b
        else:
            assert b in val and dst != b        # a product may overwrite its first operand only
            val[dst] = val[a] + val[b]; products += 1
    assert tuple(val.get(2 + i) for i in range(len(U_CHAIN_TABLE))) == U_CHAIN_TABLE
    operand = {1: 0}
    operand.update({t: 2 + i for i, t in enumerate(U_CHAIN_TABLE)})
    digits = [d for d, _ in U_CHAIN_MAIN]
    runs = [r for _, r in U_CHAIN_MAIN]
    assert digits[0] > 0 and runs[0] >= 1 and runs[-1] == 0 and all(abs(d) in operand for d in digits)
    assert all(1 <= r <= U_CHAIN_RUN_MAX for r in runs[:-1])
    acc = 0
    for d, r in U_CHAIN_MAIN:
        acc = (acc + d) << r
    assert acc == U
    squarings += sum(runs); products += len(digits) - 1
    sign = lambda d: 1 if d > 0 else -1
    return {"table": U_CHAIN_TABLE, "build": U_CHAIN_BUILD, "digits": digits, "runs": runs, "squarings": squarings, "products": products,
            "operand_digits": [sign(d) * (operand[abs(d)] + 1) for d in digits]}


# ---- built-in vectors of the device self-test (csrc/bn254_capi_selftest.hip): a 2-input Groth16 key, 64 proofs and 64 items of the two-pair check, made from the
# trapdoors so that every status is known by construction (tests/test_selftest_cpu.py holds them against the oracle).  Python integers only, like everything above.
ST_N = 64
ST_ACCEPT, ST_REJECT, ST_NOT_MEMBER, ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP, ST_PAIRING_FAILED = 1, 0, 2, 3, 4, 8
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))
HALF = (P - 1) // 2


class _Fp:
    """the two coordinate fields behind one interface, for the affine group law below"""
    zero, one = 0, 1
    mul = staticmethod(lambda a, b: a * b % P)
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    inv = staticmethod(lambda a: pow(a, -1, P))
    small = staticmethod(lambda a, k: a * k % P)


class _Fp2:
    zero, one = (0, 0), (1, 0)
    mul = staticmethod(f2mul)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % P, (a[1] + b[1]) % P))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P))
    inv = staticmethod(f2inv)
    small = staticmethod(lambda a, k: (a[0] * k % P, a[1] * k % P))


def ec_add(F, p, q):
    """affine addition on y^2 = x^3 + b (b does not enter); None is the identity"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if F.add(p[1], q[1]) == F.zero:
            return None
        lam = F.mul(F.small(F.mul(p[0], p[0]), 3), F.inv(F.small(p[1], 2)))
    else:
        lam = F.mul(F.sub(q[1], p[1]), F.inv(F.sub(q[0], p[0])))
    x = F.sub(F.sub(F.mul(lam, lam), p[0]), q[0])
    return (x, F.sub(F.mul(lam, F.sub(p[0], x)), p[1]))


def ec_mul(F, p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = ec_add(F, acc, acc)
        if bit == "1":
            acc = ec_add(F, acc, p)
    return acc


def f2sqrt(a):
    """a square root in Fp2 = Fp[i] / (i^2 + 1) by the norm method, or None"""
    def fsqrt(v):
        s = pow(v, (P + 1) // 4, P)
        return s if s * s % P == v % P else None
    n = fsqrt((a[0] * a[0] + a[1] * a[1]) % P)
    if n is None:
        return None
    for sgn in (1, -1):
        x0 = fsqrt((a[0] + sgn * n) * pow(2, -1, P) % P)
        if x0:
            y = (x0, a[1] * pow(2 * x0, -1, P) % P)
            if f2mul(y, y) == (a[0] % P, a[1] % P):
                return y
    return None


def selftest_vectors():
    import hashlib

    def rnd(tag, i=0, nonzero=True):
        c = 0
        while True:
            v = int.from_bytes(hashlib.sha256(("bn254-selftest|%s|%d|%d" % (tag, i, c)).encode()).digest(), "big") % R_ORD
            if v or not nonzero:
                return v
            c += 1

    be = lambda v: v.to_bytes(32, "big")
    G1 = (1, 2)
    g1 = lambda k: ec_mul(_Fp, G1, k % R_ORD)
    g2 = lambda k: ec_mul(_Fp2, G2_GEN, k % R_ORD)
    enc_g1 = lambda p: be(p[0]) + be(p[1])
    enc_g2 = lambda q: be(q[0][1]) + be(q[0][0]) + be(q[1][1]) + be(q[1][0])

    def cmp_g1(p):
        b = bytearray(be(p[0])); b[0] |= 0xc0 if p[1] > HALF else 0x80
        return bytes(b)

    def cmp_g2(q):      # gnark: the flag says whether y is the lexicographically larger root, by (c1, c0)
        y = q[1]
        large = y[1] > HALF if y[1] else y[0] > HALF
        b = bytearray(be(q[0][1]) + be(q[0][0])); b[0] |= 0xc0 if large else 0x80
        return bytes(b)

    # the key: beta and gamma with the halves of y.c0, y.c1 different, delta with them equal, so that the reference's reading of the compressed roots (by c0 alone)
    # and gnark's verify the same proofs (as bn254_synth_groth16 samples its keys)
    same_half = lambda q: (q[1][0] > HALF) == (q[1][1] > HALF)

    def trapdoor(tag, want_same):
        i = 0
        while True:
            k = rnd(tag, i); q = g2(k)
            if same_half(q) == want_same:
                return k, q
            i += 1
    alpha = rnd("alpha")
    beta, beta2 = trapdoor("beta", False)
    gamma, gamma2 = trapdoor("gamma", False)
    delta, delta2 = trapdoor("delta", True)
    kk = [rnd("k", i) for i in range(3)]
    vk = cmp_g1(g1(alpha)) + cmp_g1(g1(beta)) + cmp_g2(beta2) + cmp_g2(gamma2) + cmp_g1(g1(delta)) + cmp_g2(delta2) + (3).to_bytes(4, "big")
    vk += b"".join(cmp_g1(g1(k)) for k in kk) + bytes(4) + (b"\x40" + bytes(63)) * 2      # no commitments; the two points of the commitment key: the infinity flag
    # a twist point outside the r-torsion
    bt = f2mul((3, 0), f2inv(XI))
    i = 0
    while True:
        x = (rnd("bad-x0", i, False) % P, rnd("bad-x1", i, False) % P)
        y = f2sqrt(_Fp2.add(f2mul(f2mul(x, x), x), bt))
        if y is not None and ec_mul(_Fp2, (x, y), R_ORD) is not None:
            bad_b = (x, y)
            break
        i += 1
    dinv = pow(delta, -1, R_ORD)
    proofs, inputs, status = b"", b"", []
    for i in range(ST_N):
        a, b = rnd("a", i), rnd("b", i)
        xs = [rnd("x", 2 * i, False), rnd("x", 2 * i + 1, False)]
        ell = (kk[0] + xs[0] * kk[1] + xs[1] * kk[2]) % R_ORD
        c = (a * b - alpha * beta - gamma * ell) * dinv % R_ORD
        A, B, C = g1(a), g2(b), g1(c)
        st = ST_ACCEPT
        cls = (i // 8) % 5 if i % 8 == 7 else -1          # every eighth proof is corrupted, the five classes of bn254_synth_groth16 in turn
        if cls == 0:
            xs[0] += 1; st = ST_REJECT                     # (as a raw integer: stays below 2^256)
        if cls == 1:
            C = ec_add(_Fp, C, G1); st = ST_REJECT
        if cls == 3:
            B = bad_b; st = ST_NOT_IN_SUBGROUP
        rec = bytearray(enc_g1(A) + enc_g2(B) + enc_g1(C))
        if cls == 2:
            rec[32:64] = be((A[1] + 1) % P); st = ST_NOT_ON_CURVE
        if cls == 4:
            rec[0:32] = b"\xff" * 32; st = ST_NOT_MEMBER
        proofs += bytes(rec); inputs += be(xs[0]) + be(xs[1]); status.append(st)
    assert set(status) == {ST_ACCEPT, ST_REJECT, ST_NOT_MEMBER, ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP}
    # the two-pair check against the key's line tables, which hold -gamma G2 and -delta G2 (csrc/bn254_host.hpp::prepare_g16, reference mode):
    # e(a G1, -gamma G2) e(s G1, -delta G2) = 1  iff  s = -a gamma / delta
    ident = bytes(32) + be(1)                              # the identity as the workspace holds it: x = 0, y = 1, and its flag
    items, flags, p2 = b"", [], []
    for i in range(ST_N):
        a = rnd("p2", i)
        s = (-a * gamma * dinv) % R_ORD
        ok = i % 4 != 3
        p0, p1 = enc_g1(g1(a)), enc_g1(g1(s if ok else s + 1))
        fl = 0
        if i == ST_N - 6:
            p0, fl, ok = ident, 1, False                  # e(O, .) e(P_1, .) != 1
        if i == ST_N - 2:
            p0, p1, fl, ok = ident, ident, 3, True        # the empty product
        items += p0 + p1; flags.append(fl); p2.append(ST_ACCEPT if ok else ST_PAIRING_FAILED)
    return {"BN_ST_VK": vk, "BN_ST_PROOFS": proofs, "BN_ST_INPUTS": inputs, "BN_ST_STATUS": bytes(status), "BN_ST_PAIR2": items, "BN_ST_PAIR2_FLAGS": bytes(flags),
            "BN_ST_PAIR2_STATUS": bytes(p2)}


def main():
    o = []
    w = o.append
    w("// GENERATED by snark-bn254-verifier_amd/gen_constants.py -- do not edit.")
    w("// BN254 constants in 9 balanced 29-bit digits (each in [-2^28, 2^28)); field elements in Montgomery form with R = 2^261.")
    w("#pragma once")
    w("#include <stdint.h>")
    w("#define BN_NL 9")
    w("#define BN_LB 29")
    w("#define BN_MASK 0x%08xu" % MASK)
    w("#define BN_PINV 0x%08xu  /* -p^-1 mod 2^29 */" % ((-pow(P, -1, 1 << LB)) % (1 << LB)))
    w("#define BN_U_PARAM 0x%016xull /* BN parameter u */" % U)
    pl = limbs(P)
    for i, x in enumerate(pl):
        w("#define BN_P%d (%d)" % (i, x))
    w("#define BN_FP_CONST(name, ...) static const int32_t name[BN_NL] = __VA_ARGS__")
    w("BN_FP_CONST(BN_P, %s);" % arr(P))
    w("BN_FP_CONST(BN_ONE, %s);   /* R mod p */" % arr(mont(1)))
    w("BN_FP_CONST(BN_R2, %s);    /* R^2 mod p: to Montgomery form */" % arr(MONT_R * MONT_R % P))
    w("BN_FP_CONST(BN_TWO_INV, %s); /* 1/2 */" % arr(mont(pow(2, -1, P))))
    w("BN_FP_CONST(BN_THREE, %s);" % arr(mont(3)))
    w("BN_FP_CONST(BN_NINE, %s);" % arr(mont(9)))
    # twist b' = 3/xi
    bt = f2mul((3, 0), f2inv(XI))
    w("BN_FP_CONST(BN_TWIST_B0, %s);" % arr(mont(bt[0])))
    w("BN_FP_CONST(BN_TWIST_B1, %s);" % arr(mont(bt[1])))
    bt3 = f2mul((3, 0), bt)
    w("BN_FP_CONST(BN_TWIST_3B0, %s); /* 3 b' */" % arr(mont(bt3[0])))
    w("BN_FP_CONST(BN_TWIST_3B1, %s);" % arr(mont(bt3[1])))
    # Frobenius: gamma1[k] = xi^(k(p-1)/6), gamma2[k] = xi^(k(p^2-1)/6) (in Fp), gamma3[k] = xi^(k(p^3-1)/6)
    for j, name in ((1, "G1"), (2, "G2"), (3, "G3")):
        w("static const int32_t BN_FROB_%s[6][2][BN_NL] = {" % name)
        for k in range(6):
            g = f2pow(XI, k * (P**j - 1) // 6)
            w("  {%s, %s}," % (arr(mont(g[0])), arr(mont(g[1]))))
        w("};")
    # G2 generator (c0, c1 of x then y), Montgomery
    g2 = [10857046999023057135944570762232829481370756359578518086990519993285655852781,
          11559732032986387107991004021392285783925812861821192530917403151452391805634,
          8495653923123431417604973247489272438418190587263600148770280649306958101930,
          4082367875863433681332203403145435568316851327593401208105741076214120093531]
    w("static const int32_t BN_G2_GEN[4][BN_NL] = {%s};" % ", ".join(arr(mont(v)) for v in g2))
    # exponents as bit strings (MSB first, leading 1 included)
    def bits(name, e, comment):
        b = bin(e)[2:]
        w("#define %s_NBITS %d" % (name, len(b)))
        w("static const uint8_t %s_BITS[%d] = {%s}; /* %s, MSB first */" % (name, len(b), ",".join(b), comment))
    bits("BN_EXP_PM2", P - 2, "p-2 (Fermat inversion)")
    bits("BN_EXP_SQRT", (P + 1) // 4, "(p+1)/4 (square root, p = 3 mod 4)")
    bits("BN_EXP_PM3O4", (P - 3) // 4, "(p-3)/4 (Fp2 square root)")
    bits("BN_EXP_PM1O2", (P - 1) // 2, "(p-1)/2")
    bits("BN_EXP_U", U, "u")
    # NAF of 6u+2, most significant digit first, leading digit (1) included
    n = naf(6 * U + 2)[::-1]
    assert n[0] == 1
    w("#define BN_ATE_NAF_LEN %d" % len(n))
    w("static const int8_t BN_ATE_NAF[%d] = {%s}; /* NAF(6u+2), MSB first */" % (len(n), ",".join(str(d) for d in n)))
    w("#define BN_ATE_STEPS %d /* doublings + additions after the leading digit + 2 Frobenius steps */"
      % ((len(n) - 1) + sum(1 for d in n[1:] if d) + 2))
    nu = naf(U)[::-1]
    w("#define BN_U_NAF_LEN %d" % len(nu))
    w("static const int8_t BN_U_NAF[%d] = {%s}; /* NAF(u), MSB first */" % (len(nu), ",".join(str(d) for d in nu)))
    # the addition-subtraction chain of exp-by-u in the final exponentiation (u_chain below; bn254_vm.h::vm_exp_u runs it)
    c = u_chain()
    w("/* x^u on the cyclotomic subgroup as an addition-subtraction chain (tools/search_u_chain.py): %d squarings + %d products." % (c["squarings"], c["products"]))
    w("   Operands: 0 = x (the source), 1 = the temporary (the destination, free until the accumulator starts), 2 + i = table entry i.")
    w("   BN_U_CHAIN_BUILD: the table, one step {op, dst, a, b} each: op 0: dst <- a^(2^b) (b squarings, one run), op 1: dst <- a * b.")
    w("   BN_U_CHAIN_DIGIT / _RUN, MSB first: the accumulator starts as the operand of digit 0; then `run` squarings and a product with the")
    w("   operand of the next digit, conjugated (= inverted) where the digit is negative.  A digit is +-(operand + 1); no run exceeds %d. */" % U_CHAIN_RUN_MAX)
    w("#define BN_U_CHAIN_TABLE_LEN %d" % len(c["table"]))
    w("static const uint8_t BN_U_CHAIN_TABLE[%d] = {%s}; /* exponents of the table entries */" % (len(c["table"]), ",".join(str(t) for t in c["table"])))
    w("#define BN_U_CHAIN_BUILD_LEN %d" % len(c["build"]))
    w("static const uint8_t BN_U_CHAIN_BUILD[%d][4] = {%s};" % (len(c["build"]), ",".join("{%d,%d,%d,%d}" % st for st in c["build"])))
    w("#define BN_U_CHAIN_LEN %d" % len(c["digits"]))
    w("static const int8_t BN_U_CHAIN_DIGIT[%d] = {%s}; /* %s */" % (len(c["digits"]), ",".join(str(d) for d in c["operand_digits"]), " ".join("%+d" % d for d in c["digits"])))
    w("static const uint8_t BN_U_CHAIN_RUN[%d] = {%s}; /* squarings after the digit */" % (len(c["runs"]), ",".join(str(r) for r in c["runs"])))
    # modulus r for host-side scalar handling (plain 32-bit words, little endian)
    w("static const uint32_t BN_R_WORDS[8] = {%s};" % ", ".join("0x%08xu" % ((R_ORD >> (32 * i)) & 0xffffffff) for i in range(8)))
    w("static const uint32_t BN_P_WORDS[8] = {%s};" % ", ".join("0x%08xu" % ((P >> (32 * i)) & 0xffffffff) for i in range(8)))
    w("static const uint32_t BN_P_HALF_WORDS[8] = {%s}; /* (p-1)/2 */" % ", ".join("0x%08xu" % ((((P - 1) // 2) >> (32 * i)) & 0xffffffff) for i in range(8)))
    # the self-test's tables: seen only by the translation unit that asks for them
    w("#if defined(BN254_SELFTEST_TABLES)")
    w("/* Built-in vectors of the device self-test (bn254_capi_selftest.hip; include/bn254_verify.h, bn254_device_selftest): a 2-input Groth16 key in gnark's bytes,")
    w("   %d raw proofs with their inputs and statuses (every eighth corrupted: input + 1, C + G1, A.y + 1, B outside G2, A.x >= p), and %d items P_0 | P_1 of the" % (ST_N, ST_N))
    w("   two-pair check against the key's line tables (flags: bit t = P_t is the identity) with ACCEPT or BN254_ERR_PAIRING_FAILED. */")
    w("#define BN_ST_N %d" % ST_N)
    for name, data in selftest_vectors().items():
        w("static const uint8_t %s[%d] = {" % (name, len(data)))
        for i in range(0, len(data), 32):
            w("  " + ",".join("0x%02x" % b for b in data[i:i + 32]) + ",")
        w("};")
    w("#endif")
    sys.stdout.write("\n".join(o) + "\n")


if __name__ == "__main__":
    main()
