"""AddressSanitizer + UndefinedBehaviorSanitizer over everything of this repository that runs on a CPU --
sanitizers on the CPU builds only, the GPU pool has none:
  * the oracle (oracle/*.c) and the host build of the product's arithmetic headers with the bound tracker (tests/hostsim) rebuilt with -fsanitize=address,undefined
    and run through their own test files in a child interpreter that preloads the sanitizer runtimes;
  * the HOST HALF OF THE PRODUCT -- csrc/bn254_capi*.hip with its parsers, key preparation, plans, pinned ring, context pools and thread pool -- compiled with g++
    against a host-memory stand-in for the HIP runtime (tests/hostsan) and driven through the C ABI: malformed-bytes fuzz of the three parsers that take
    attacker-shaped lengths (groth16/converter.rs:28-65, plonk/converter.rs:18-119, the SP1 fixture reader), batches around every plan boundary on the fake
    device, the RLC fallback, wide keys, PlonK calls in flight, compressed proofs on both sides of the 2^20 chunk, the SP1 entries of both protocols with every vkey
    stride, an allocation failure at every allocation of a call of each kind.
A report aborts (-fno-sanitize-recover).  First run: one real finding, a left shift of a negative int in the inner loop of the constant-time inversion
(bn254_fp.h, bn254_plonk.hpp: undefined before C++20), fixed."""
import os
import platform
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runtime(name):
    p = subprocess.check_output(["gcc", "-print-file-name=" + name], text=True).strip()
    assert os.path.isabs(p) and os.path.exists(p), "sanitizer runtime %s not found" % name
    return p


def test_oracle_and_hostsim_under_asan_ubsan():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "liboracle_san.so"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim"), "HSFLAGS=-DHS_WITH_CURVE", "libhostsim_san.so"])
    env = dict(os.environ, LD_PRELOAD=_runtime("libasan.so") + ":" + _runtime("libubsan.so"), ASAN_OPTIONS="detect_leaks=0",
               BN254_ORACLE_LIB=os.path.join(ROOT, "oracle", "liboracle_san.so"), BN254_HOSTSIM_LIB="libhostsim_san.so")
    files = ["tests/test_oracle_golden.py", "tests/test_oracle_arith.py", "tests/test_hostsim.py", "tests/test_rlc_hostsim.py", "tests/test_msm_rows.py"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_host_half_of_the_library_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "hostsan")
    exe = os.path.join(d, "hostsan")
    src = [os.path.join(d, "hostsan_main.cpp"), os.path.join(d, "hip", "hip_runtime.h")] + [os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc", f)
                                                                                            for f in os.listdir(os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                               "-x", "c++", "-I", d, "-I", os.path.join(ROOT, "include"), os.path.join(d, "hostsan_main.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=d)
    # leak detection ON: the allocation-failure loops of the harness make every allocation of a call fail in turn, and whatever an aborted call leaves behind
    # must still be owned by a handle (found that way: a retry after a partly failed table upload overwrote -- leaked -- the tables already uploaded)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden"), "100"], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan ok" in r.stdout and "LeakSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]


def test_threaded_host_paths_under_tsan():
    """ThreadSanitizer over the host code that runs several threads: bn254_groth16_verify_batch_multi / bn254_plonk_verify_batch_multi on EIGHT
    fake devices -- the `w > 1` branch no one-GPU box takes: one host thread per device, per-device contexts of one shared key, a failing device -- concurrent callers on one
    key and one device, the key caches of the single-proof entries under contention, PlonK calls in flight on the context pool, the process-wide host thread pool.  Same
    harness as the ASan build (tests/hostsan), its threaded scenarios alone; a report makes the run fail (halt_on_error)."""
    d = os.path.join(ROOT, "tests", "hostsan")
    exe = os.path.join(d, "hostsan_tsan")
    src = [os.path.join(d, "hostsan_main.cpp"), os.path.join(d, "hip", "hip_runtime.h")] + [os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc", f)
                                                                                            for f in os.listdir(os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc")) if f.endswith((".h", ".hpp", ".hip"))]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBN_HOST_PLAIN_INLINE", "-fsanitize=thread", "-fno-omit-frame-pointer",
                               "-x", "c++", "-I", d, "-I", os.path.join(ROOT, "include"), os.path.join(d, "hostsan_main.cpp"), "-o", exe, "-lpthread", "-ldl"], cwd=d)
    # started with address-space randomisation off (setarch -R, this child only): the ThreadSanitizer of GCC 11 aborts with "unexpected memory mapping" under the
    # wider mmap randomisation of newer kernels, before the harness runs
    r = subprocess.run(["setarch", platform.machine(), "-R", exe, os.path.join(ROOT, "tests", "golden"), "10", "threads"], cwd=ROOT, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "hostsan ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
