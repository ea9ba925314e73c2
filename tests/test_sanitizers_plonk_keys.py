"""The host code of the PlonK batches over many keys (csrc/bn254_capi_plonk_keys.hip: the cache of key sets with its lock, the pool of pass contexts and of call
buffers, the pinned ring of the host entry, the hook of bn254_plonk_vk_free) under AddressSanitizer + UndefinedBehaviorSanitizer with leak detection, and its
concurrent scenarios under ThreadSanitizer.  tests/hostsan/hostsan_plonk_keys.cpp is the harness: a stand-alone program, the host half of the library as one
translation unit against the stand-in HIP runtime of tests/hostsan, the real grouping (csrc/bn254_keys.h compiled for the host), stand-in launchers that read
every byte the kernels read."""
import os
import platform
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_plonk_keys.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_plonk_keys.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_plonk_key_sets_under_asan_ubsan():
    """batches around the granule and the pass cut through both entries, lists that name a handle twice, more lists than cache slots, a member freed and a new list
    built, refused calls, an allocation failure at every allocation of a reservation and of a batch, then the concurrent scenarios; leak detection on: whatever a
    dropped or evicted set held must have been released"""
    exe = os.path.join(D, "hostsan_plonk_keys")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "6"], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_plonk_keys ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]


def test_plonk_key_sets_under_tsan():
    """four host threads: the same list from two of them (host and device entry), changing lists on both fake devices from a third, and one that frees and
    re-prepares a member of its own lists meanwhile (started with address-space randomisation off, as tests/test_sanitizers.py does for this compiler)"""
    exe = os.path.join(D, "hostsan_plonk_keys_tsan")
    _build(exe, ["-fsanitize=thread"])
    r = subprocess.run(["setarch", platform.machine(), "-R", exe, "6", "threads"], cwd=ROOT, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_plonk_keys ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
