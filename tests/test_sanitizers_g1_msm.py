"""The host code of the G1 multi-scalar multiplication (csrc/bn254_capi_g1msm.hip: bn254_g1_bases_prepare, _free, _count, bn254_g1_msm_batch, _device,
bn254_g1_msm_reserve -- the argument checks, the handle, items staged at a padded length, term records, rows, scratch and result words sized by the shape, the pass
size, every error path) TOGETHER WITH the bodies of the two new kernels (csrc/bn254_g1msm.h::g1msm_load_item and g1msm_store_item, compiled for the host in the
launchers' place) and the probe's host compile under AddressSanitizer + UndefinedBehaviorSanitizer with leak detection.  tests/hostsan/hostsan_g1_msm.cpp is the
harness, a program of its own against the stand-in HIP runtime of tests/hostsan.  Nothing is loaded into python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_g1_msm.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    src.append(os.path.join(ROOT, "include", "bn254_verify.h"))
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_g1_msm.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_g1_msm_under_asan_ubsan():
    """the argument checks of the six entries; a handle prepared, used, refused on another device and above its count, freed while another lives; host calls of three
    passes (BN254_G1_MSM_PASS=1000) at five shapes, packed and padded, exact and strict; the probe's host compile in four forms; the device entry at and above a
    reservation (nothing allocated at or below it) at an odd output address; an allocation failure at every allocation of bn254_g1_bases_prepare and of a call of the
    largest shape, each followed by the same call answering right (nothing leaked); two host threads with different shapes on one device"""
    exe = os.path.join(D, "hostsan_g1_msm")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", BN254_G1_MSM_PASS="1000"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_g1_msm ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
