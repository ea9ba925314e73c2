"""What the PlonK stage kernels must leave for a proof, stated without the stage source (helper of test_plonk_stage_values_cpu.py and
test_gpu_plonk_stage_values.py; not a test): the ChaCha20 streams of the KZG batching scalar and of the BN254_FLAG_RLC weight, the BSB22 hash-to-field, and the
per-proof record of bn254_dbg_plonk_stages from oracle calls alone -- O.plonk_verify (status), O.plonk_stage_digests (zeta), O.plonk_pairing_inputs_lam (P0, P1),
O.g1_mul (the weighted form)."""
import hashlib
import struct

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ACCEPT, OPENING_MISMATCH, PAIRING_FAILED = 1, 7, 8
OFF_CLAIMED = 516
RLC_NONCE_TWIST = 0x00524c43      # "RLC" in nonce word 2: the weight stream is not the lambda stream
ZERO32, ZERO64 = bytes(32), bytes(64)


def chacha_block(key, counter, nonce):
    """The ChaCha20 block function (RFC 8439 section 2.3): key 32 bytes, nonce 12 bytes -> 16 words."""
    def rotl(x, n):
        return ((x << n) | (x >> (32 - n))) & 0xffffffff

    def qr(s, a, b, c, d):
        s[a] = (s[a] + s[b]) & 0xffffffff; s[d] = rotl(s[d] ^ s[a], 16)
        s[c] = (s[c] + s[d]) & 0xffffffff; s[b] = rotl(s[b] ^ s[c], 12)
        s[a] = (s[a] + s[b]) & 0xffffffff; s[d] = rotl(s[d] ^ s[a], 8)
        s[c] = (s[c] + s[d]) & 0xffffffff; s[b] = rotl(s[b] ^ s[c], 7)

    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + list(struct.unpack("<8I", key)) + [counter] + list(struct.unpack("<3I", nonce))
    s = list(init)
    for _ in range(10):
        qr(s, 0, 4, 8, 12); qr(s, 1, 5, 9, 13); qr(s, 2, 6, 10, 14); qr(s, 3, 7, 11, 15)
        qr(s, 0, 5, 10, 15); qr(s, 1, 6, 11, 12); qr(s, 2, 7, 8, 13); qr(s, 3, 4, 9, 14)
    return [(a + b) & 0xffffffff for a, b in zip(s, init)]


def _key_nonce(words, twist=0):
    assert len(words) == 11 and all(0 <= w < 1 << 32 for w in words)
    return struct.pack("<8I", *words[:8]), struct.pack("<3I", words[8], words[9], words[10] ^ twist)


def lam_of(words, i):
    """lambda of slot i under the 11-word key: the first four words of blocks 3i, 3i + 1, 3i + 2, each little-endian, the 48 bytes read big-endian, mod r."""
    key, nonce = _key_nonce(words)
    b = b"".join(struct.pack("<4I", *chacha_block(key, 3 * i + j, nonce)[:4]) for j in range(3))
    return int.from_bytes(b, "big") % R


def weight_of(words, i):
    """the BN254_FLAG_RLC weight of slot i: the first four words of block i of the stream with the twisted nonce, word 0 forced odd and least significant."""
    key, nonce = _key_nonce(words, RLC_NONCE_TWIST)
    w = chacha_block(key, i, nonce)[:4]
    return (w[0] | 1) | w[1] << 32 | w[2] << 64 | w[3] << 96


def expand_message_xmd(msg, dst, n):
    """RFC 9380 section 5.3.1 with SHA-256 (b = 32 bytes, input block 64 bytes), as oracle/protocol.c states it."""
    ell = (n + 31) // 32
    assert ell <= 255 and len(dst) <= 255
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + n.to_bytes(2, "big") + b"\0" + dst_prime).digest()
    bs = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        bs.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, bs[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(bs)[:n]


def h2f_bytes(commitment64):
    return expand_message_xmd(commitment64, b"BSB22-Plonk", 48)


def h2f(commitment64):
    return int.from_bytes(h2f_bytes(commitment64), "big") % R


def commitments(proof, n_qcp):
    """the BSB22 commitments of a raw proof: behind the 6 + n_qcp claimed values, the opening at zeta omega (64 + 32 bytes) and their count"""
    off = OFF_CLAIMED + 32 * (6 + n_qcp) + 100
    return [proof[off + 64 * k:off + 64 * (k + 1)] for k in range(n_qcp)]


def check_h2f(O, proof, vk, inputs, n_qcp):
    """pins the restatement to the oracle's 48 bytes of commitment 0 (and, for the reference's fixture, to the golden of test_oracle_golden.py through the caller)"""
    st, dg = O.plonk_stage_digests(proof, vk, [int.from_bytes(x, "big") for x in inputs])
    assert n_qcp >= 1 and dg["h2f"] == h2f_bytes(commitments(proof, n_qcp)[0]), "hash-to-field restatement differs from the oracle"
    return dg["h2f"]


def be32(v):
    return int(v).to_bytes(32, "big")


def on_curve(p64):
    x, y = int.from_bytes(p64[:32], "big"), int.from_bytes(p64[32:], "big")
    return x < P and y < P and (y * y - x * x * x - 3) % P == 0


def expect(O, vk, proof, inputs, n_qcp, lam, weight=None, slot=None):
    """The record bn254_dbg_plonk_stages must give for this proof under this lambda (weight: the weighted form), as the dict binding._plonk_stage_records makes --
    without "lin", which no oracle call gives.  Three oracle calls: the status under lam, the stage digests, the pairing operands under lam."""
    ints = [int.from_bytes(x, "big") for x in inputs]
    st = O.plonk_verify(proof, vk, inputs, lam=lam)
    _, dg = O.plonk_stage_digests(proof, vk, ints)
    base = {"zeta": be32(int.from_bytes(dg["zeta"], "big") % R), "h2f0": dg["h2f"], "ints": ints}
    alive = st in (ACCEPT, PAIRING_FAILED)
    e = {"status1": ACCEPT if alive else st, "status": ACCEPT if alive else st, "lin_inf": 0, "p0_inf": 0, "p1_inf": 0, "zeta": ZERO32, "lambda": ZERO32,
         "lin_opening": ZERO32, "h2f": [ZERO32] * 8, "p0": ZERO64, "p1": ZERO64, "pad": bytes(7), "oracle_status": st}
    if slot is not None:
        e["slot"] = slot
    if alive or st == OPENING_MISMATCH:
        e["zeta"] = base["zeta"]
    if not alive:
        return e
    st_l, (p0, p1), _ = O.plonk_pairing_inputs_lam(proof, vk, base["ints"], lam)
    assert st_l == st
    e["lambda"] = be32(lam)
    e["lin_opening"] = proof[OFF_CLAIMED:OFF_CLAIMED + 32]        # the free identity: the stage's value IS the first claimed value wherever the opening check passed
    cs = commitments(proof, n_qcp)
    if n_qcp:
        assert base["h2f0"] == h2f_bytes(cs[0])
    e["h2f"] = [be32(h2f(c)) for c in cs] + [ZERO32] * (8 - n_qcp)
    if p0 == ZERO64 and p1 == ZERO64:
        e["ambiguous"] = True          # the oracle writes nothing when either operand is the identity: the probe's flags decide (compare() asks for one at least)
        return e
    if weight is not None:
        p0, p1 = O.g1_mul(p0, weight), O.g1_mul(p1, weight)
    e["p0"], e["p1"] = p0, p1
    return e


def compare(got, want, what=""):
    """every field of a probe record against its expectation, byte for byte"""
    for k, v in want.items():
        if k in ("oracle_status", "ambiguous"):
            continue
        if want.get("ambiguous") and k in ("p0", "p1", "p0_inf", "p1_inf"):
            continue
        assert got[k] == v, "%s: %s differs: got %r, expected %r (oracle status %d)" % (what, k, got[k], v, want["oracle_status"])
    if want.get("ambiguous"):
        assert got["p0_inf"] or got["p1_inf"], what
        assert (got["p0"] == ZERO64) == bool(got["p0_inf"]) and (got["p1"] == ZERO64) == bool(got["p1_inf"]), what
    if want["status1"] == ACCEPT:
        assert got["lin_inf"] == 0 and on_curve(got["lin"]) and got["lin"] != ZERO64, "%s: the digest of the linearised polynomial is no curve point" % what
    else:
        assert got["lin"] == ZERO64, what


def rows(inputs, n_public, i):
    return [inputs[32 * (n_public * i + j):32 * (n_public * i + j + 1)] for j in range(n_public)]
