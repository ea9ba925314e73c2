"""The synthetic PlonK workload generator (bn254_synth_plonk, _range, _for_inputs in csrc/bn254_capi_dbg.hip: the key and its trapdoors, the per-proof scalar
arithmetic, the layout of keys, records, strides and input rows, the worker threads, every argument error) under AddressSanitizer + UndefinedBehaviorSanitizer with
leak detection.  tests/hostsan/hostsan_synth_plonk.cpp is the harness, a program of its own: the host half of the library as one translation unit against the
stand-in HIP runtime of tests/hostsan.  Nothing is loaded into python under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = os.path.join(ROOT, "tests", "hostsan")


def _build(exe, flags):
    csrc = os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")
    src = [os.path.join(D, f) for f in ("hostsan_synth_plonk.cpp", "hostsan_main.cpp", os.path.join("hip", "hip_runtime.h"))] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE"] + flags + ["-fno-omit-frame-pointer", "-x", "c++", "-I", D, "-I", os.path.join(ROOT, "include"),
                               os.path.join(D, "hostsan_synth_plonk.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=D)


def test_synth_plonk_under_asan_ubsan():
    """five key shapes and a domain of exactly n_public + n_qcp rows, every second proof corrupted, buffers of exactly the documented sizes; a stride larger than the
    proof; n = 0; a range against its slice; proofs for chosen rows; each proof through the host compile of the verifier's first stage; the argument errors on
    one-byte buffers"""
    exe = os.path.join(D, "hostsan_synth_plonk")
    _build(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan_synth_plonk ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
