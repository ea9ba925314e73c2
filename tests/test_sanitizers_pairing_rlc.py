"""The host code of BN254_FLAG_RLC on the pairing batch (csrc/bn254_capi_pairing_rlc.hip: bn254_pairing_check_batch_flags, _device, the knob, the counters, the probe --
the argument checks, the group buffers sized in the ensure step, a host call staged with the records in front of the items and the probe's weights behind them, every
error path) TOGETHER WITH the BN_HD bodies of the new kernels (csrc/bn254_pairing_rlc.h: the weight step, the Miller run over the variable positions, the group sums,
product and check, through the probe's host compile) under AddressSanitizer + UndefinedBehaviorSanitizer with leak detection.  tests/hostsan/hostsan_pairing_rlc.cpp is
the harness, a program of its own against the stand-in HIP runtime of tests/hostsan.  Nothing is loaded into python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_pairing_rlc.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    src.append(os.path.join(ROOT, "include", "bn254_verify.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_pairing_rlc.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_pairing_rlc_under_asan_ubsan():
    """the knob's clamps; the argument checks of both entries (unknown flag bits, those of the shared entry); host calls of three passes (BN254_PAIRING_PASS=1000) at four
    shapes, packed and padded, with the counters of every call; the knob above n (the exact launches, out[3] alone); the device entry at and above a reservation, at an odd
    status address and with a corrupted record; the probe's host compile on real items at four shapes and the probe on a stand-in device; an allocation failure at every
    allocation of a call, each followed by the same call answering right (nothing leaked); two host threads on one device while the knob moves"""
    exe = os.path.join(D, "hostsan_pairing_rlc")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", BN254_PAIRING_PASS="1000"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_pairing_rlc ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
