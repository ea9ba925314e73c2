#!/usr/bin/env python3
"""PlonK batches over many verifying keys against what a caller did before them.  Device-resident, distinct proofs of shape (2 public inputs, 1 BSB22 commitment,
2^26 rows), all valid, every key with its own seed and so its own SRS, proofs assigned to keys uniformly.
Per cell (n proofs, K keys), alternating in one process, REPS times each:
  A  bn254_plonk_verify_batch_keys_device: one call, the proofs in shuffled order
  B  K calls of bn254_plonk_verify_batch_device, one per key, proofs pre-sorted by key (the sort is not charged), every key's tables resident
  C  the single-key entry on n proofs of one key: the ceiling
  L  (--lane) A with bn254_set_plonk_keys_params(0): every pass in the lane form of the pairing check, what a list ran before the cooperative form
  R  (--rlc) A with BN254_FLAG_RLC (honoured from bn254_set_plonk_rlc_params' pass size on; the default threshold unless --rlc-min), and CR: C with the flag
--coop-max V sets the knob of A's passes (default: the library's).  --invalid-every N plants an invalid proof every N (statuses against the generator's).
A library without the knobs (BN254_LIB_PATH: the build of an earlier revision) runs A, B and C only.
Prints one line per cell (median and min .. max of the repetitions, milliseconds; spread = (max - min) / median) and one JSON line at the end.

  python tools/bench_plonk_keys.py [--reps 5] [--sizes 4096,65536,262144] [--keys 1,4,16,64] [--rlc] [--rlc-min N] [--lane] [--coop-max V] [--invalid-every N] [--no-b]"""
import argparse, importlib, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # loads the HIP runtime torch ships before the library does
pkg = importlib.import_module("snark-bn254-verifier_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="4096,65536,262144")
ap.add_argument("--keys", default="1,4,16,64")
ap.add_argument("--rlc", action="store_true")
ap.add_argument("--rlc-min", type=int, default=-1)
ap.add_argument("--lane", action="store_true")
ap.add_argument("--coop-max", type=int, default=-1)
ap.add_argument("--invalid-every", type=int, default=0)
ap.add_argument("--no-b", action="store_true", help="leave the one-call-per-key column out")
args = ap.parse_args()
HAS_KNOBS = hasattr(pkg.lib(), "bn254_set_plonk_keys_params")
if not HAS_KNOBS:
    print("# this library has no bn254_set_plonk_keys_params: columns A, B, C only", flush=True)
    args.rlc = args.lane = False
else:
    pkg.set_plonk_keys_params(args.coop_max)
    pkg.set_plonk_rlc_params(args.rlc_min)
    COOP_MAX = pkg.dbg_plonk_keys_knobs()[0]
    print("# coop_max %d, rlc from %d slots per pass" % pkg.dbg_plonk_keys_knobs(), flush=True)
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
    vk, proofs, inputs, exp = pkg.synth_plonk(0x9D0000 + k, SHAPE[0], SHAPE[1], SHAPE[2], count, invalid_every=args.invalid_every, threads=16)
    return (vk, torch.frombuffer(bytearray(proofs), dtype=torch.uint8).view(count, PLEN), torch.frombuffer(bytearray(inputs), dtype=torch.uint8).view(count, 64),
            torch.frombuffer(bytearray(exp), dtype=torch.uint8))


results = []
t0 = time.perf_counter()
vk0, c_p, c_i, c_e = gen(0, n_max)          # key 0's own stream: what C verifies at every K, and key 0's share of A and B
pvks = {0: pkg.PreparedPlonkVk(vk0)}
print("# key 0: %d proofs generated in %.1f s" % (n_max, time.perf_counter() - t0), flush=True)
for K in key_counts:
    # key k's proofs [0, n_max / K): the cells of a smaller n take a prefix of every key's stream
    t0 = time.perf_counter()
    per_max = n_max // K
    parts = []
    parts.append((c_p[:per_max], c_i[:per_max], c_e[:per_max]))
    for k in range(1, K):
        vk, p_k, i_k, e_k = gen(k, per_max)
        if k not in pvks:
            pvks[k] = pkg.PreparedPlonkVk(vk)
        parts.append((p_k, i_k, e_k))
    print("# K = %d: %d proofs generated in %.1f s" % (K, per_max * K, time.perf_counter() - t0), flush=True)
    for n in sizes:
        if n % K:
            continue
        per = n // K
        d_sorted_p = torch.cat([p[:per] for p, _, _ in parts]).to(dev).contiguous()
        d_sorted_i = torch.cat([i[:per] for _, i, _ in parts]).to(dev).contiguous()
        want_sorted = int(sum(int((e[:per] == pkg.ACCEPT).sum()) for _, _, e in parts))      # ACCEPTs the generator expects: of the mixed batch, of key 0's stream
        want_c = want_sorted if K == 1 else int((c_e[:n] == pkg.ACCEPT).sum())
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

        def run_a(flags=0):
            ks.verify_batch_device(d_idx.data_ptr(), d_p.data_ptr(), d_i.data_ptr(), d_st.data_ptr(), n, proof_stride=PLEN, input_stride=64, stream=sp, flags=flags)

        def run_l():
            pkg.set_plonk_keys_params(0)
            try:
                run_a()
            finally:
                pkg.set_plonk_keys_params(COOP_MAX)

        def run_r():
            run_a(pkg.FLAG_RLC)

        def run_cr():
            pvks[0].verify_batch_device(d_c_p.data_ptr(), d_c_i.data_ptr(), d_st.data_ptr(), n, proof_stride=PLEN, stream=sp, flags=pkg.FLAG_RLC)

        def run_b():
            for k in range(K):
                pvks[k].verify_batch_device(d_sorted_p.data_ptr() + PLEN * per * k, d_sorted_i.data_ptr() + 64 * per * k, d_st.data_ptr() + per * k, per, proof_stride=PLEN, stream=sp)

        def run_c():      # n valid proofs of key 0's own stream
            pvks[0].verify_batch_device(d_c_p.data_ptr(), d_c_i.data_ptr(), d_st.data_ptr(), n, proof_stride=PLEN, stream=sp)

        runs = (("A", run_a),) + (() if args.no_b else (("B", run_b),)) + (("C", run_c),) + ((("L", run_l),) if args.lane else ()) + ((("R", run_r), ("CR", run_cr)) if args.rlc else ())
        state0 = ks.state() if HAS_KNOBS else None
        for name, fn in runs:             # warm-up of every shape, and the statuses
            d_st.fill_(0xEE)
            timed(fn)
            ok = int((d_st == pkg.ACCEPT).sum())
            assert ok == (want_c if name in ("C", "CR") else want_sorted), (name, ok)
        ms = {name: [] for name, _ in runs}
        for _ in range(args.reps):
            for name, fn in runs:
                ms[name].append(timed(fn))
        out = {"n": n, "keys": K}
        for name in ms:
            med = statistics.median(ms[name])
            out[name] = {"median_ms": med, "min_ms": min(ms[name]), "max_ms": max(ms[name]), "spread": (max(ms[name]) - min(ms[name])) / med, "mproofs_per_s": n / med / 1e3}
        ratios = [("A", "C")] + ([("B", "A")] if "B" in ms else []) + ([("L", "A")] if "L" in ms else []) + ([("A", "R"), ("C", "CR")] if "R" in ms else [])
        for x, y in ratios:
            out["%s_over_%s" % (x, y)] = out[x]["median_ms"] / out[y]["median_ms"]
        if HAS_KNOBS:
            out["state_delta"] = [b - a for a, b in zip(state0, ks.state())]      # joint passes, groups, failed groups, cooperative per-proof checks (warm-up included)
        print("n = %7d  K = %3d  " % (n, K) + "  ".join("%s %8.2f ms (%.2f .. %.2f, spread %.3f)" % (k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"], out[k]["spread"]) for k in ms) +
              "  " + "  ".join("%s/%s %.3f" % (x, y, out["%s_over_%s" % (x, y)]) for x, y in ratios) + ("  state %s" % out["state_delta"] if HAS_KNOBS else ""), flush=True)
        results.append(out)
        del d_sorted_p, d_sorted_i, d_p, d_i, d_idx, d_st, d_c_p, d_c_i, ks
    del parts
print(json.dumps({"bench": "plonk_keys", "reps": args.reps, "shape": SHAPE, "invalid_every": args.invalid_every, "knobs": list(pkg.dbg_plonk_keys_knobs()) if HAS_KNOBS else None, "cells": results}))
