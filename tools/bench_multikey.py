#!/usr/bin/env python3
"""Batches over many verifying keys against what a caller did before them.  Device-resident inputs, 2-input keys, all proofs valid, proofs assigned to keys uniformly.
Per cell (n proofs, K keys), alternating in one process, REPS times each:
  A  bn254_groth16_verify_batch_keys_device: one call, the proofs in shuffled order
  B  K calls of bn254_groth16_verify_batch_device on the same library, one per key, proofs pre-sorted by key (the sort is not charged), one stream, every key's tables
     resident.  B needs each key's own 13-bit window tables on the device (39 MB per 2-input key), so it runs on at most 256 distinct keys; for K = 4096 it times 256
     of the 4096 calls and the figure is that time x 16 (marked "scaled")
  C  the single-key entry on n proofs of one key: the ceiling
Prints one line per cell (median and min .. max of the repetitions, milliseconds) and one JSON line at the end.

  python tools/bench_multikey.py [--reps 5] [--sizes 1048576,65536] [--keys 1,16,256,4096]
  python tools/bench_multikey.py --trace      # one A (K = 256) and one C run at n = 2^20 and nothing else: the run to put under rocprofv3 --kernel-trace --stats"""
import argparse, importlib, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # loads the HIP runtime torch ships before the library does
pkg = importlib.import_module("snark-bn254-verifier_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="1048576,65536")
ap.add_argument("--keys", default="1,16,256,4096")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream(dev)
B_MAX_KEYS = 256
sizes = [1 << 20] if args.trace else [int(x) for x in args.sizes.split(",")]
key_counts = [256] if args.trace else [int(x) for x in args.keys.split(",")]
max_keys = max(key_counts)

t0 = time.perf_counter()
with ThreadPoolExecutor(16) as pool:      # key preparation is host work (the line tables): 6 ms a key
    vks = list(pool.map(lambda k: pkg.synth_groth16(0x9B0000 + k, 2, 0, invalid_every=0, agree=True, threads=1)[0], range(max_keys)))
    pvks = list(pool.map(pkg.PreparedVk, vks))
print("# %d keys prepared in %.1f s" % (max_keys, time.perf_counter() - t0), flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    stream.synchronize()
    return (time.perf_counter() - t) * 1e3


def cell(n, K):
    per = n // K
    assert per * K == n
    # proofs sorted by key (what B is handed), then the same records shuffled for A
    parts = [pkg.synth_groth16(0x9B0000 + k, 2, per, invalid_every=0, agree=True, threads=16) for k in range(K)]
    d_sorted_p = torch.frombuffer(bytearray(b"".join(p[1] for p in parts)), dtype=torch.uint8).to(dev).view(n, 256)
    d_sorted_i = torch.frombuffer(bytearray(b"".join(p[2] for p in parts)), dtype=torch.uint8).to(dev).view(n, 64)
    del parts
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(n + K))
    d_p, d_i = d_sorted_p[perm].contiguous(), d_sorted_i[perm].contiguous()
    d_idx = (perm // per).to(torch.int32).contiguous()
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    ks = pkg.KeySet(pvks[:K])
    ks.reserve(n)
    kb = min(K, B_MAX_KEYS)
    for k in range(kb):
        pvks[k].reserve(per)
    pvks[0].reserve(n)
    sp = stream.cuda_stream

    def run_a():
        ks.verify_batch_device(d_idx.data_ptr(), d_p.data_ptr(), d_i.data_ptr(), d_st.data_ptr(), n, input_stride=64, stream=sp)

    def run_b():
        for k in range(kb):
            pvks[k].verify_batch_device(d_sorted_p.data_ptr() + 256 * per * k, d_sorted_i.data_ptr() + 64 * per * k, d_st.data_ptr() + per * k, per, 256, 2, 0, sp)

    def run_c():      # n records "of one key": the first key's `per` proofs are valid, the rest are other keys' (REJECT): the same work per proof
        pvks[0].verify_batch_device(d_sorted_p.data_ptr(), d_sorted_i.data_ptr(), d_st.data_ptr(), n, 256, 2, 0, sp)

    runs = (("A", run_a), ("C", run_c)) if args.trace else (("A", run_a), ("B", run_b), ("C", run_c))
    for name, fn in runs:             # warm-up of every shape, and the statuses
        d_st.fill_(0xEE)
        timed(fn)
        ok = int((d_st == pkg.ACCEPT).sum())
        want = n if name == "A" else per * kb if name == "B" else per
        assert ok == want, (name, ok, want)
    ms = {name: [] for name, _ in runs}
    for _ in range(1 if args.trace else args.reps):
        for name, fn in runs:
            ms[name].append(timed(fn))
    scale = K / kb
    out = {"n": n, "keys": K, "b_scaled_by": scale}
    for name in ms:
        f = scale if name == "B" else 1.0
        out[name] = {"median_ms": statistics.median(ms[name]) * f, "min_ms": min(ms[name]) * f, "max_ms": max(ms[name]) * f}
    if "B" in out:
        out["B_over_A"] = out["B"]["median_ms"] / out["A"]["median_ms"]
    out["A_over_C"] = out["A"]["median_ms"] / out["C"]["median_ms"]
    print("n = %8d  K = %5d  " % (n, K) + "  ".join("%s %8.2f ms (%.2f .. %.2f)%s" % (k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"], " scaled x%d" % scale if k == "B" and scale > 1 else "")
                                                     for k in ms) + ("  B/A %.2f" % out["B_over_A"] if "B" in out else "") + "  A/C %.3f" % out["A_over_C"], flush=True)
    return out


results = [cell(n, K) for n in sizes for K in key_counts if n % K == 0]
print(json.dumps({"bench": "multikey", "reps": args.reps, "cells": results}))
