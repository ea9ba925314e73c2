#!/usr/bin/env python3
"""PlonK batches over many verifying keys against what a caller did before them.  Device-resident, distinct proofs of shape (2 public inputs, 1 BSB22 commitment,
2^26 rows), all valid, every key with its own seed and so its own SRS, proofs assigned to keys uniformly.
Per cell (n proofs, K keys), alternating in one process, REPS times each:
  A  bn254_plonk_verify_batch_keys_device: one call, the proofs in shuffled order
  B  K calls of bn254_plonk_verify_batch_device, one per key, proofs pre-sorted by key (the sort is not charged), every key's tables resident
  C  the single-key entry on n proofs of one key: the ceiling
Prints one line per cell (median and min .. max of the repetitions, milliseconds; spread = (max - min) / median) and one JSON line at the end.

  python tools/bench_plonk_keys.py [--reps 5] [--sizes 4096,65536,262144] [--keys 1,4,16,64]"""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # loads the HIP runtime torch ships before the library does
pkg = importlib.import_module("snark-bn254-verifier_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="4096,65536,262144")
ap.add_argument("--keys", default="1,4,16,64")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream(dev)
sizes = [int(x) for x in args.sizes.split(",")]
key_counts = [int(x) for x in args.keys.split(",")]
SHAPE, PLEN = (2, 1, 26), 904
n_max = max(sizes)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()                      # the PlonK entries are host-synchronous
    return (time.perf_counter() - t) * 1e3


def gen(k, count):
    vk, proofs, inputs, _ = pkg.synth_plonk(0x9D0000 + k, SHAPE[0], SHAPE[1], SHAPE[2], count, invalid_every=0, threads=16)
    return vk, torch.frombuffer(bytearray(proofs), dtype=torch.uint8).view(count, PLEN), torch.frombuffer(bytearray(inputs), dtype=torch.uint8).view(count, 64)


results = []
t0 = time.perf_counter()
vk0, c_p, c_i = gen(0, n_max)          # key 0's own stream: what C verifies at every K, and key 0's share of A and B
pvks = {0: pkg.PreparedPlonkVk(vk0)}
print("# key 0: %d proofs generated in %.1f s" % (n_max, time.perf_counter() - t0), flush=True)
for K in key_counts:
    # key k's proofs [0, n_max / K): the cells of a smaller n take a prefix of every key's stream
    t0 = time.perf_counter()
    per_max = n_max // K
    parts = []
    parts.append((c_p[:per_max], c_i[:per_max]))
    for k in range(1, K):
        vk, p_k, i_k = gen(k, per_max)
        if k not in pvks:
            pvks[k] = pkg.PreparedPlonkVk(vk)
        parts.append((p_k, i_k))
    print("# K = %d: %d proofs generated in %.1f s" % (K, per_max * K, time.perf_counter() - t0), flush=True)
    for n in sizes:
        if n % K:
            continue
        per = n // K
        d_sorted_p = torch.cat([p[:per] for p, _ in parts]).to(dev).contiguous()
        d_sorted_i = torch.cat([i[:per] for _, i in parts]).to(dev).contiguous()
        perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(n + K))
        d_p, d_i = d_sorted_p[perm].contiguous(), d_sorted_i[perm].contiguous()
        d_idx = (perm // per).to(torch.int32).contiguous()
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        d_c_p, d_c_i = (d_sorted_p, d_sorted_i) if K == 1 else (c_p[:n].to(dev).contiguous(), c_i[:n].to(dev).contiguous())
        ks = pkg.PlonkKeySet([pvks[k] for k in range(K)])
        ks.reserve(n, proof_stride=PLEN)
        for k in range(K):
            pvks[k].reserve(per)
        pvks[0].reserve(n)
        sp = stream.cuda_stream

        def run_a():
            ks.verify_batch_device(d_idx.data_ptr(), d_p.data_ptr(), d_i.data_ptr(), d_st.data_ptr(), n, proof_stride=PLEN, input_stride=64, stream=sp)

        def run_b():
            for k in range(K):
                pvks[k].verify_batch_device(d_sorted_p.data_ptr() + PLEN * per * k, d_sorted_i.data_ptr() + 64 * per * k, d_st.data_ptr() + per * k, per, proof_stride=PLEN, stream=sp)

        def run_c():      # n valid proofs of key 0's own stream
            pvks[0].verify_batch_device(d_c_p.data_ptr(), d_c_i.data_ptr(), d_st.data_ptr(), n, proof_stride=PLEN, stream=sp)

        runs = (("A", run_a), ("B", run_b), ("C", run_c))
        for name, fn in runs:             # warm-up of every shape, and the statuses
            d_st.fill_(0xEE)
            timed(fn)
            ok = int((d_st == pkg.ACCEPT).sum())
            assert ok == n, (name, ok)
        ms = {name: [] for name, _ in runs}
        for _ in range(args.reps):
            for name, fn in runs:
                ms[name].append(timed(fn))
        out = {"n": n, "keys": K}
        for name in ms:
            med = statistics.median(ms[name])
            out[name] = {"median_ms": med, "min_ms": min(ms[name]), "max_ms": max(ms[name]), "spread": (max(ms[name]) - min(ms[name])) / med, "mproofs_per_s": n / med / 1e3}
        out["B_over_A"] = out["B"]["median_ms"] / out["A"]["median_ms"]
        out["A_over_C"] = out["A"]["median_ms"] / out["C"]["median_ms"]
        print("n = %7d  K = %3d  " % (n, K) + "  ".join("%s %8.2f ms (%.2f .. %.2f, spread %.3f)" % (k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"], out[k]["spread"]) for k in ms) +
              "  B/A %.2f  A/C %.3f" % (out["B_over_A"], out["A_over_C"]), flush=True)
        results.append(out)
        del d_sorted_p, d_sorted_i, d_p, d_i, d_idx, d_st, d_c_p, d_c_i, ks
    del parts
print(json.dumps({"bench": "plonk_keys", "reps": args.reps, "shape": SHAPE, "cells": results}))
