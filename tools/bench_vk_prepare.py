#!/usr/bin/env python3
"""Preparing many Groth16 verifying keys: bn254_groth16_vk_prepare_batch (one call, the per-key work on the device) against the same keys through
bn254_groth16_vk_prepare, one call per key -- on ONE host thread (a C or Rust caller's loop) and on 16 host threads (what tools/bench_multikey.py did before the batch
entry).  Wall time of the whole preparation, handles freed outside the timed window; every method is warmed once, then the methods ALTERNATE for --reps repetitions in
one process; median and min .. max are printed.

Workloads: 1, 2, 4, 8, 16, 64, 256, 4096 and 65 536 two-input keys, and 16 keys of 1024 inputs.  The lists cycle through at most 4096 distinct synthetic keys (neither
path keeps anything between keys, so a repeated key costs what a new one costs).  A host loop that would run for more than --loop-budget seconds is timed on a prefix
of the list and scaled (marked "scaled"): its cost per key does not depend on the list.
Per-stage device times of the batch entry come from HIP events around its launches (bn254_dbg_g16_vk_prepare_batch), summed over the passes of one call.
Prints one line per workload, the crossovers, and one JSON line at the end.

  python tools/bench_vk_prepare.py [--reps 5] [--sizes 1,16,256,4096,65536] [--loop-budget 6]"""
import argparse, importlib, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # loads the HIP runtime torch ships before the library does
pkg = importlib.import_module("snark-bn254-verifier_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="1,2,4,8,16,64,256,4096,65536")
ap.add_argument("--loop-budget", type=float, default=6.0)
ap.add_argument("--no-wide", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
sizes = [int(x) for x in args.sizes.split(",")]
DISTINCT = 4096


def free(keys):
    for k in keys:
        if k is not None:
            k.close()


def t_batch(vks):
    t = time.perf_counter()
    keys = pkg.prepare_vks(vks, pkg.VK_REFERENCE, 0)
    dt = time.perf_counter() - t
    assert all(k is not None for k in keys)
    free(keys)
    return dt


def t_loop(vks, threads, pool):
    t = time.perf_counter()
    keys = [pkg.PreparedVk(v) for v in vks] if threads == 1 else list(pool.map(pkg.PreparedVk, vks))
    dt = time.perf_counter() - t
    free(keys)
    return dt


def stats(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs)}


def fmt(s):
    return "%10.2f (%9.2f .. %9.2f)" % (s["median_ms"], s["min_ms"], s["max_ms"])


def measure(label, vks, pool, per_key_s):
    """per_key_s: {threads: seconds per key of the host loop, from the workloads before} -- decides how long a prefix of the list the loops are timed on"""
    n = len(vks)
    prefix = {}
    for th in (1, 16):
        est = per_key_s.get(th)
        m = n if est is None or est * n <= args.loop_budget else max(16 * th, int(args.loop_budget / est))
        prefix[th] = min(n, m)
    t_batch(vks); t_loop(vks[:prefix[1]], 1, pool); t_loop(vks[:prefix[16]], 16, pool)          # warm-up of every method at this shape
    tb, t1, t16 = [], [], []
    for _ in range(args.reps):
        tb.append(t_batch(vks))
        t1.append(t_loop(vks[:prefix[1]], 1, pool) * n / prefix[1])
        t16.append(t_loop(vks[:prefix[16]], 16, pool) * n / prefix[16])
    keys, status, stage = pkg.dbg_prepare_vks(vks, pkg.VK_REFERENCE, 0)
    assert status == [0] * n
    free(keys)
    row = {"workload": label, "keys": n, "batch": stats(tb), "loop_1_thread": stats(t1), "loop_16_threads": stats(t16),
           "loop_1_thread_scaled_from": prefix[1] if prefix[1] < n else None, "loop_16_threads_scaled_from": prefix[16] if prefix[16] < n else None,
           "speedup_vs_1_thread": statistics.median(t1) / statistics.median(tb), "speedup_vs_16_threads": statistics.median(t16) / statistics.median(tb), "stage_ms": stage}
    per_key_s[1] = statistics.median(t1) / n; per_key_s[16] = statistics.median(t16) / n
    print("%-22s batch %s ms | loop, 1 thread %s ms%s x%7.2f | loop, 16 threads %s ms%s x%7.2f" % (
        label, fmt(row["batch"]), fmt(row["loop_1_thread"]), " scaled" if prefix[1] < n else "       ", row["speedup_vs_1_thread"],
        fmt(row["loop_16_threads"]), " scaled" if prefix[16] < n else "       ", row["speedup_vs_16_threads"]), flush=True)
    print("%-22s   device stages of one batch call, ms: %s" % ("", "  ".join("%s %.3f" % (k, v) for k, v in stage.items())), flush=True)
    return row


print("# %s, %s, torch %s; times are wall milliseconds of the whole preparation: median (min .. max) of %d alternating repetitions after one warm-up each" % (
    torch.cuda.get_device_name(0), pkg.lib().bn254_version().decode(), torch.__version__, args.reps), flush=True)
t0 = time.perf_counter()
with ThreadPoolExecutor(16) as pool:
    distinct = list(pool.map(lambda k: pkg.synth_groth16(0x9C0000 + k, 2, 0, invalid_every=0, agree=True, threads=1)[0], range(min(max(sizes), DISTINCT))))
    print("# %d distinct 2-input keys made in %.1f s" % (len(distinct), time.perf_counter() - t0), flush=True)
    rows, per_key = [], {}
    for n in sizes:
        rows.append(measure("%d x 2 inputs" % n, [distinct[i % len(distinct)] for i in range(n)], pool, per_key))
    if not args.no_wide:
        wide = list(pool.map(lambda k: pkg.synth_groth16(0x9C8000 + k, 1024, 0, invalid_every=0, agree=True, threads=1)[0], range(16)))
        rows.append(measure("16 x 1024 inputs", wide, pool, {}))
cross = {}
for name, key in (("1 thread", "speedup_vs_1_thread"), ("16 threads", "speedup_vs_16_threads")):
    two = [r for r in rows if r["workload"].endswith("x 2 inputs")]
    wins = [r["keys"] for r in two if r[key] > 1.0]
    loses = [r["keys"] for r in two if r[key] <= 1.0]
    first = min([k for k in wins if all(k > l for l in loses)] or [None], key=lambda x: (x is None, x))
    cross[name] = first
    print("# against the host loop on %s the batch entry wins from %s two-input keys on (measured sizes: %s)" % (name, first, ", ".join(str(r["keys"]) for r in two)), flush=True)
print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows, "wins_from_keys": cross}))
