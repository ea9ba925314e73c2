"""SP1 test data shared by tests/test_sp1_cpu.py and tests/test_gpu_sp1.py: the public values of the SP1 v2.0.0 fixtures (tests/golden/sp1/*.bin, bincode
SP1ProofWithPublicValues) and the digest rule in plain Python."""
import hashlib
import os
import struct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sp1")
NAMES = ["fibonacci", "is-prime", "sha2", "tendermint"]
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def digest(pv):
    """committed_values_digest: SHA-256 with the top three bits of byte 0 cleared."""
    d = bytearray(hashlib.sha256(bytes(pv)).digest())
    d[0] &= 0x1F
    return bytes(d)


def parse(buf):
    """(variant, raw proof, public inputs (2 x 32 bytes), vkey hash, public values) of one fixture file."""
    off = 0

    def u32():
        nonlocal off
        v = struct.unpack_from("<I", buf, off)[0]; off += 4
        return v

    def u64():
        nonlocal off
        v = struct.unpack_from("<Q", buf, off)[0]; off += 8
        return v

    def blob():
        nonlocal off
        k = u64(); b = buf[off:off + k]; off += k
        return b

    variant = u32()
    s0, s1, _enc, raw = blob(), blob(), blob(), blob()
    vkey_hash = buf[off:off + 32]; off += 32
    for _ in range(u64()):                 # stdin: Vec<Vec<u8>>
        blob()
    u64()                                  # ptr
    assert u64() == 0                      # proofs: empty
    pv = blob()                            # public values
    assert blob() == b"v2.0.0"             # sp1_version
    assert off == len(buf), (off, len(buf))
    inputs = int(s0).to_bytes(32, "big") + int(s1).to_bytes(32, "big")
    return variant, bytes.fromhex(raw.decode()), inputs, bytes(vkey_hash), bytes(pv)


def fixture(name, kind):
    with open(os.path.join(GOLDEN, "%s_%s_proof.bin" % (name, kind)), "rb") as f:
        return parse(f.read())
