"""The host half of the device self-test -- the gate in front of every path that makes a device ready, the per-device state, the entries, the comparison
(csrc/bn254_capi_selftest.hip) -- under AddressSanitizer + UndefinedBehaviorSanitizer with leak detection, and its concurrent scenario under ThreadSanitizer.
tests/hostsan/hostsan_selftest.cpp is the harness: a stand-alone program, the one-unit host build of tests/hostsan/hostsan_main.cpp with a stand-in for the device
half of the self-test that fails check 4 on one of eight fake devices."""
import os
import platform
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_selftest.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_selftest.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_selftest_gate_under_asan_ubsan():
    """six host threads make first calls on eight fake devices at once: exactly one run per device, device 3 (whose check 4 disagrees) refuses every Groth16 and PlonK
    entry with BN254_E_SELFTEST and writes no status byte, the others verify; an explicit run clears the failure once the device agrees again; a fault injection leaves
    a recorded state alone unless asked to record; an allocation failure at every allocation of a run, explicit and automatic, leaves the state and the allocation
    count as they were; leak detection on"""
    exe = os.path.join(D, "hostsan_selftest")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "hostsan_selftest ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]


def test_selftest_gate_under_tsan():
    """the concurrent scenario alone (started with address-space randomisation off, as tests/test_sanitizers.py does for this compiler)"""
    exe = os.path.join(D, "hostsan_selftest_tsan")
    _build(exe, ["-fsanitize=thread"])
    r = subprocess.run(["setarch", platform.machine(), "-R", exe, os.path.join(ROOT, "tests", "golden"), "threads"], cwd=ROOT,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "hostsan_selftest ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
