"""The host code of SMALL batches over many keys -- the direct form of csrc/bn254_capi_keys.hip, its plan (csrc/bn254_g16_plan.h::g16_keys_form) and its knob
(bn254_set_keys_params) -- under AddressSanitizer + UndefinedBehaviorSanitizer with leak detection, and its concurrent scenario under ThreadSanitizer.
tests/hostsan/hostsan_keys_small.cpp is the harness: the one-unit host build of tests/hostsan/hostsan_keys.cpp with stand-ins for all three launchers of the key-set
path and the knob turned to 30 720 (a host build starts at 0, which is what keeps the older harness on the grouped form)."""
import os
import platform
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_keys_small.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_keys_small.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_small_key_sets_under_asan_ubsan():
    """n in {1, 5, 6, 300, 30720, 30721} through both entries with raw and compressed records (the last one takes the grouped form), an index outside the list, a
    reservation smaller than a later batch, a device call after a reservation that allocates nothing, the knob flipped between batches on one cached list, an
    allocation failure at every allocation of a direct-form batch, then the concurrent scenario; leak detection on"""
    exe = os.path.join(D, "hostsan_keys_small")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "8"], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_keys_small ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]


def test_small_key_sets_under_tsan():
    """the six host threads of tests/test_sanitizers_multikey.py with the knob on, one of them moving it meanwhile (started with address-space randomisation off, as
    tests/test_sanitizers.py does for this compiler)"""
    exe = os.path.join(D, "hostsan_keys_small_tsan")
    _build(exe, ["-fsanitize=thread"])
    r = subprocess.run(["setarch", platform.machine(), "-R", exe, "8", "threads"], cwd=ROOT, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_keys_small ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
