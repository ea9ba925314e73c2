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
  python tools/bench_multikey.py --trace      # one A (K = 256) and one C run at n = 2^20 and nothing else: the run to put under rocprofv3 --kernel-trace --stats

--small measures the SMALL batches (n = 256 .. 30 720; K = 1, 16, 256, min(n, 4096); one more row with 16-input keys at n = 4096, K = 16), where a batch over many
keys takes one of two forms (bn254_set_keys_params):
  A1  the direct cooperative form (the knob at its maximum)
  A0  the grouped lane form (the knob at 0)
  C   the single-key entry on n proofs
A library without bn254_set_keys_params (BN254_LIB_PATH: the build of an earlier revision, the baseline) has one form; its column is A.

  python tools/bench_multikey.py --small [--reps 5]
  python tools/bench_multikey.py --small --trace     # one A1 batch and one C batch at n = 4096 (K = 256, then 16-input keys with K = 16) and nothing else"""
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
ap.add_argument("--small", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream(dev)
B_MAX_KEYS = 256
sizes = [1 << 20] if args.trace else [int(x) for x in args.sizes.split(",")]
key_counts = [256] if args.trace else [int(x) for x in args.keys.split(",")]
max_keys = max(key_counts)

if args.small:
    sizes = [4096] if args.trace else [256, 1024, 4096, 16384, 30720]
    key_counts = [256] if args.trace else [1, 16, 256, 4096]
    max_keys = max(min(n, K) for n in sizes for K in key_counts)
try:
    pkg.set_keys_params(-1)
    HAVE_KNOB = True
except AttributeError:                    # a library of a revision without the direct form
    HAVE_KNOB = False

t0 = time.perf_counter()
with ThreadPoolExecutor(16) as pool:      # (making the synthetic keys is host work)
    vks = list(pool.map(lambda k: pkg.synth_groth16(0x9B0000 + k, 2, 0, invalid_every=0, agree=True, threads=1)[0], range(max_keys)))
def prepare(vks):
    """one call, on the device (bn254_groth16_vk_prepare_batch; tools/bench_vk_prepare.py measures it against the per-key host loop)"""
    try:
        return pkg.prepare_vks(vks, device=0)
    except AttributeError:                # a library of a revision without the entry (BN254_LIB_PATH): the host loop on 16 threads
        with ThreadPoolExecutor(16) as pool:
            return list(pool.map(pkg.PreparedVk, vks))


pvks = prepare(vks)
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


def small_cell(n, K, n_public, keys):
    """proof i under key i % K (uniform; the counts differ by one where K does not divide n), in shuffled order"""
    per = (n + K - 1) // K
    parts = [pkg.synth_groth16(0x9B0000 + 4096 * (n_public != 2) + k, n_public, per, invalid_every=0, agree=True, threads=16 if K <= 16 else 2) for k in range(K)]
    order = torch.randperm(n, generator=torch.Generator().manual_seed(n + K)).tolist()
    rec = bytearray(256 * n); rows = bytearray(32 * n_public * n); idx = []
    for pos, i in enumerate(order):
        k, j = i % K, i // K
        rec[256 * pos:256 * pos + 256] = parts[k][1][256 * j:256 * j + 256]
        rows[32 * n_public * pos:32 * n_public * (pos + 1)] = parts[k][2][32 * n_public * j:32 * n_public * (j + 1)]
        idx.append(k)
    del parts
    d_p = torch.frombuffer(rec, dtype=torch.uint8).to(dev); d_i = torch.frombuffer(rows, dtype=torch.uint8).to(dev)
    d_idx = torch.tensor(idx, dtype=torch.int32).to(dev)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    ks = pkg.KeySet(keys[:K])
    ks.reserve(n)
    keys[0].reserve(n)
    sp = stream.cuda_stream

    def run_a():
        ks.verify_batch_device(d_idx.data_ptr(), d_p.data_ptr(), d_i.data_ptr(), d_st.data_ptr(), n, input_stride=32 * n_public, stream=sp)

    def run_c():      # n records "of one key": the same work per proof whatever the verdict
        keys[0].verify_batch_device(d_p.data_ptr(), d_i.data_ptr(), d_st.data_ptr(), n, 256, n_public, 0, sp)

    def with_knob(v):
        def run():
            pkg.set_keys_params(v)
            run_a()
        return run

    runs = [("A1", with_knob(30720)), ("A0", with_knob(0))] if HAVE_KNOB else [("A", run_a)]
    runs = (runs[:1] if args.trace else runs) + [("C", run_c)]
    for name, fn in runs:             # warm-up of every shape, and the statuses
        d_st.fill_(0xEE)
        timed(fn)
        if name != "C":
            assert int((d_st == pkg.ACCEPT).sum()) == n, name
            if HAVE_KNOB:
                assert ks.last_form() == (1 if name == "A1" else 0), name
    ms = {name: [] for name, _ in runs}
    for _ in range(1 if args.trace else args.reps):
        for name, fn in runs:
            ms[name].append(timed(fn))
    out = {"n": n, "keys": K, "n_public": n_public}
    for name in ms:
        out[name] = {"median_ms": statistics.median(ms[name]), "min_ms": min(ms[name]), "max_ms": max(ms[name])}
    print("n = %6d  K = %5d  inputs %2d  " % (n, K, n_public) + "  ".join("%s %7.3f ms (%.3f .. %.3f)" % (k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"]) for k in ms), flush=True)
    return out


if args.small:
    results = []
    for n in sizes:
        for K in sorted({min(n, K) for K in key_counts}):
            results.append(small_cell(n, K, 2, pvks))
    with ThreadPoolExecutor(16) as pool:
        vks16 = list(pool.map(lambda k: pkg.synth_groth16(0x9B0000 + 4096 + k, 16, 0, invalid_every=0, agree=True, threads=1)[0], range(16)))
    pvks16 = prepare(vks16)
    results.append(small_cell(4096, 16, 16, pvks16))
    if HAVE_KNOB:
        pkg.set_keys_params(30720)
    print(json.dumps({"bench": "multikey_small", "reps": args.reps, "knob": HAVE_KNOB, "lib": os.path.basename(os.path.dirname(pkg.lib_path())), "cells": results}))
    sys.exit(0)

results = [cell(n, K) for n in sizes for K in key_counts if n % K == 0]
print(json.dumps({"bench": "multikey", "reps": args.reps, "cells": results}))
