"""BN254_FLAG_RLC over PlonK key lists (csrc/bn254_capi_plonk_keys.hip::pk_run_pass: the weighted stage 2, the group sums, the joint check with the key per group,
the read-back and the exact check behind a failed group; the counters of bn254_plonk_keys_state and the two knobs) under AddressSanitizer +
UndefinedBehaviorSanitizer with leak detection, and its concurrent scenario under ThreadSanitizer.  tests/hostsan/hostsan_plonk_keys_rlc.cpp is the harness: a
stand-alone program, the host half of the library as one translation unit against the stand-in HIP runtime of tests/hostsan, stand-in launchers that touch every
byte the kernels touch.  Nothing loaded into Python runs under a sanitizer."""
import os
import platform
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_plonk_keys_rlc.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_plonk_keys_rlc.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_plonk_key_sets_rlc_under_asan_ubsan():
    """passes with the flag through both entries with and without failed groups, in one chain and in two, the counters of the state against the stand-ins' own
    counts, the flag below the threshold, the setters' clamps, a freed member, an allocation failure at every allocation of a batch with the flag, then the
    concurrent scenario; leak detection on"""
    exe = os.path.join(D, "hostsan_plonk_keys_rlc")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "6"], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_plonk_keys_rlc ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]


def test_plonk_key_sets_rlc_under_tsan():
    """two host threads on one list, one with the flag and one without, and a third on changing lists on both fake devices (started with address-space
    randomisation off, as tests/test_sanitizers.py does for this compiler)"""
    exe = os.path.join(D, "hostsan_plonk_keys_rlc_tsan")
    _build(exe, ["-fsanitize=thread"])
    r = subprocess.run(["setarch", platform.machine(), "-R", exe, "6", "threads"], cwd=ROOT, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_plonk_keys_rlc ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
