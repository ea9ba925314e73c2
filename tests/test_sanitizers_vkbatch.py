"""The host code of bn254_groth16_vk_prepare_batch (csrc/bn254_capi_vkbatch.hip: the scan of every key, the gathering of a pass, the staging buffers, the images and
the handles it makes, every error path) TOGETHER WITH the bodies of its kernels (csrc/bn254_vkprep.h, compiled for the host in the launcher's place) under
AddressSanitizer + UndefinedBehaviorSanitizer with leak detection.  tests/hostsan/hostsan_vkbatch.cpp is the harness, a program of its own: the host half of the
library as one translation unit against the stand-in HIP runtime of tests/hostsan.  Nothing is loaded into python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_vkbatch.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_vkbatch.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_vk_prepare_batch_under_asan_ubsan():
    """good lists in both modes on both fake devices, a malformed-bytes fuzz of whole lists (truncations, flipped bits, attacker-shaped K and commitment-index counts,
    flag bits) held to the single-key entry key by key, an allocation failure at every allocation of a call (every out[i] NULL, nothing leaked), argument errors"""
    exe = os.path.join(D, "hostsan_vkbatch")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "40"], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_vkbatch ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
