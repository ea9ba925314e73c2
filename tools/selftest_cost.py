#!/usr/bin/env python3
"""Cost of the device self-test (include/bn254_verify.h, bn254_device_selftest) on the GPU of this machine, as profiles/selftest_cost.txt records it:
  1. six explicit runs in one process with the time between the events around each check (the first run is the process's first use of the device);
  2. the first-call latency of a fresh process -- library load, then one single-proof bn254_groth16_verify with an uncached key, then a second call -- five processes
     each for this build, this build with BN254_SELFTEST=0 and, with --parent-lib, a library built from the parent commit.
  python tools/selftest_cost.py [--parent-lib PATH] [--out FILE]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS = os.path.join(ROOT, "snark-bn254-verifier_amd", "libbn254_verify_amd.so")
NAMES = ["fp", "fp12_lane", "fp12_coop", "pairing_lane", "g16_lane", "g16_coop", "pair2_lane", "pair2_coop", "codec", "sha256", "key+tables"]
lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)

CHILD = r'''
import ctypes as C, sys, time, json
blob = open(sys.argv[2], "rb").read()
import struct
lv, = struct.unpack("<I", blob[:4]); vk = blob[4:4+lv]; proof = blob[4+lv:4+lv+256]; inputs = blob[4+lv+256:4+lv+256+64]
st = (C.c_uint8 * 1)(0xEE)
t0 = time.perf_counter()
L = C.CDLL(sys.argv[1])
t1 = time.perf_counter()
rc = L.bn254_groth16_verify(proof, C.c_size_t(256), vk, C.c_size_t(len(vk)), inputs, C.c_size_t(2), C.c_uint(0), st)
t2 = time.perf_counter()
rc2 = L.bn254_groth16_verify(proof, C.c_size_t(256), vk, C.c_size_t(len(vk)), inputs, C.c_size_t(2), C.c_uint(0), st)
t3 = time.perf_counter()
state = -9
if hasattr(L, "bn254_device_selftest_state"):
    s = C.c_int(); L.bn254_device_selftest_state(0, C.byref(s), None); state = s.value
print(json.dumps({"rc": rc, "status": st[0], "load_ms": (t1 - t0) * 1e3, "first_ms": (t2 - t1) * 1e3, "second_ms": (t3 - t2) * 1e3, "state": state}))
'''

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libbn254_verify_amd.so built from the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    OUT = tempfile.mkdtemp(prefix="selftest_cost_")
    L = C.CDLL(THIS)
    # vectors for the first-call children: one valid proof
    n_public = 2
    L.bn254_synth_groth16_vk_len.restype = C.c_size_t
    lv = L.bn254_synth_groth16_vk_len(C.c_size_t(n_public))
    vk = (C.c_uint8 * lv)(); pr = (C.c_uint8 * 256)(); inp = (C.c_uint8 * 64)(); ex = (C.c_uint8 * 1)()
    assert L.bn254_synth_groth16(C.c_uint64(0xC057), C.c_size_t(2), C.c_size_t(1), 0, 1, 1, vk, pr, inp, ex) == 0
    import struct
    blob_path = os.path.join(OUT, "first_call_blob.bin")
    open(blob_path, "wb").write(struct.pack("<I", lv) + bytes(vk) + bytes(pr) + bytes(inp))
    child_path = os.path.join(OUT, "first_call_child.py")
    open(child_path, "w").write(CHILD)
    say("# Cost of the device self-test (bn254_device_selftest) on one MI355X")
    say("## 1. explicit runs in one process (the first is the process's first use of the device: code objects load, the host computes its expected values)")
    rows = []
    for i in range(6):
        mask, ms = C.c_uint(9), C.c_float()
        rc = L.bn254_device_selftest(0, C.byref(mask), C.byref(ms))
        g = (C.c_float * 11)(); h = C.c_float(); w = C.c_float()
        L.bn254_dbg_selftest_ms(g, C.byref(h), C.byref(w))
        assert rc == 0 and mask.value == 0, (rc, mask.value)
        rows.append((ms.value, list(g), h.value))
        say("run %d: wall %.2f ms, host work meanwhile %.2f ms, between events: %s" % (i, ms.value, h.value, " ".join("%s %.2f" % (NAMES[k], g[k]) for k in range(11))))
    later = rows[1:]
    say("median of runs 1..5: wall %.2f ms; per check (ms): %s" % (statistics.median(r[0] for r in later),
        " ".join("%s %.2f" % (NAMES[k], statistics.median(r[1][k] for r in later)) for k in range(11))))
    say("first run: wall %.2f ms, host work (key, expected values) %.2f ms, overlapped with the device" % (rows[0][0], rows[0][2]))
    say()
    say("## 2. first-call latency: fresh process, library load -> first status byte of one single-proof bn254_groth16_verify (uncached key), then a second call")
    for label, lib, env in (("parent commit", args.parent_lib, {}), ("this commit", THIS, {}), ("this commit, BN254_SELFTEST=0", THIS, {"BN254_SELFTEST": "0"})):
        if not lib:
            continue
        res = []
        for i in range(5):
            e = dict(os.environ); e.pop("BN254_SELFTEST", None); e.update(env)
            r = subprocess.run([sys.executable, child_path, lib, blob_path], capture_output=True, text=True, timeout=120, env=e)
            if r.returncode != 0:
                say("%s: child failed: %s" % (label, (r.stdout + r.stderr)[-500:])); sys.exit(1)
            d = json.loads(r.stdout.strip().splitlines()[-1])
            assert d["rc"] == 0 and d["status"] == 1, d
            res.append(d)
        say("%s: load %s ms | first call %s ms (median %.1f) | second call %s ms | self-test state after: %s" % (
            label, " ".join("%.1f" % d["load_ms"] for d in res), " ".join("%.1f" % d["first_ms"] for d in res), statistics.median(d["first_ms"] for d in res),
            " ".join("%.2f" % d["second_ms"] for d in res), res[0]["state"]))
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
