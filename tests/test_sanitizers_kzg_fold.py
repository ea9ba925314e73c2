"""The host code of the KZG batch-opening entries (csrc/bn254_capi_kzg.hip: bn254_kzg_verify_folded_batch, _device, bn254_kzg_fold_reserve -- the argument checks,
records staged at a padded length behind the key, term records, rows and scratch sized by the number of digests, the pass size, the weighted path, every error path)
TOGETHER WITH the loader's body (csrc/bn254_kzg.h::kzg_fold_load_record, compiled for the host in the launcher's place) and the probe's host compile under
AddressSanitizer + UndefinedBehaviorSanitizer with leak detection.  tests/hostsan/hostsan_kzg_fold.cpp is the harness, a program of its own against the stand-in HIP
runtime of tests/hostsan.  Nothing is loaded into python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_kzg_fold.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    src.append(os.path.join(ROOT, "include", "bn254_verify.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_kzg_fold.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_kzg_fold_under_asan_ubsan():
    """the argument checks; host calls of three passes (BN254_PAIRING_PASS=1000) at k = 1, 3 and the largest k, packed and padded, record lengths that are and are not
    multiples of 4, exact and strict; the probe's host compile; the device entry at and above a reservation (nothing allocated at or below it) and with a corrupted
    key; the weighted path with a failing group and its counters; an allocation failure at every allocation of an exact and of a weighted call at the largest k, each
    followed by the same call answering right (nothing leaked); two host threads with different k on one device"""
    exe = os.path.join(D, "hostsan_kzg_fold")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", BN254_PAIRING_PASS="1000"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_kzg_fold ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
