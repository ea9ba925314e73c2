"""The host code of the pairing batch with shared, prepared G2 points (csrc/bn254_capi_pairing.hip: bn254_g2_prepare, the argument checks of the _shared entries, the
prepared records staged in front of every pass's items, the per-device workspace and its lock, every error path) TOGETHER WITH the bodies of its kernels
(csrc/bn254_pairing_batch.h::pb_item_shared_on_host, compiled for the host in the launcher's place) under AddressSanitizer + UndefinedBehaviorSanitizer with leak
detection.  tests/hostsan/hostsan_pairing_shared.cpp is the harness, a program of its own against the stand-in HIP runtime of tests/hostsan.  Nothing is loaded into
python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_pairing_shared.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    src.append(os.path.join(ROOT, "include", "bn254_verify.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_pairing_shared.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_pairing_shared_under_asan_ubsan():
    """bn254_g2_prepare into a block of exactly the record's size; the argument checks; host calls of three passes (BN254_PAIRING_PASS=1000) at three masks with packed
    and padded items, the records staged with every pass; the device entry at and above a reservation and with a corrupted record; an allocation failure at every
    allocation of a call, each followed by the same call answering right (nothing leaked); two host threads on one device with different masks"""
    exe = os.path.join(D, "hostsan_pairing_shared")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", BN254_PAIRING_PASS="1000"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_pairing_shared ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
