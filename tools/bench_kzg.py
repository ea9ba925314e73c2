#!/usr/bin/env python3
"""Times of the KZG batch (bn254_kzg_verify_batch_device) on one GPU: device-resident openings at n in {4096, 65536, 262144}, the exact entry and the entry with
BN254_FLAG_RLC honoured (bn254_set_kzg_params(64)) ALTERNATING call by call in one session, and beside them bn254_pairing_check_batch_shared_device on the same openings
restated as items (F_i, -H_i) with F_i precomputed on the host -- the pairing alone, the floor of the exact entry.
  python tools/bench_kzg.py [--sizes 4096,65536,262144] [--steps 5] [--out profiles/r17_kzg_batch.txt]
The openings are --distinct (default 512) valid openings of random cubic polynomials under a key with known trapdoors, tiled to n: the kernels' work does not depend on
the values, and a valid batch never reaches the fallback of the weighted path (its best case; a failed group adds the per-opening check of its wavefront).  Every call
is timed on its own from the call to the status bytes on the device, after one warm-up call and a reservation; the median of --steps calls is reported with its
min .. max.  Writes the table to --out and prints one JSON line.
  python tools/bench_kzg.py --digests 1,4,8 [--data-len 0] [--sizes 4096,65536] [--out profiles/r18_kzg_fold.txt]
times bn254_kzg_verify_folded_batch_device instead (batch-opening records of K digests, valid, --distinct of them tiled), exact and with the flag honoured, alternating
call by call with bn254_kzg_verify_batch_device on plain openings at the same n; per size it also reports the cost per further digest (the slope of the medians over K)."""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default=None, help="default: 4096,65536,262144; with --digests 4096,65536")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--digests", type=str, default=None, help="K or a list K1,K2,..: time the batch-opening entry at these numbers of digests")
    ap.add_argument("--data-len", type=int, default=0)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r18_kzg_fold.txt" if args.digests else "r17_kzg_batch.txt")
    if args.sizes is None:
        args.sizes = "4096,65536" if args.digests else "4096,65536,262144"
    if args.digests:
        return main_fold(args)
    import torch
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    from oracle import oracle as O
    O.build(); O.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sizes = [int(x) for x in args.sizes.split(",")]
    rng = random.Random(0x17)
    s, tau = rng.randrange(2, R), rng.randrange(2, R)
    gen = O.g1_gen()
    g1_of = lambda a: bytes(64) if a % R == 0 else O.g1_mul(gen, a % R)
    neg = lambda p: p if p == bytes(64) else p[:32] + ((P - int.from_bytes(p[32:], "big")) % P).to_bytes(32, "big")
    g2, tau_g2 = O.g2_gen(), O.g2_mul(O.g2_gen(), tau)
    st, key = pkg.kzg_key_prepare(g1_of(s), g2, tau_g2)
    assert st == pkg.ACCEPT
    recs = pkg.g2_prepare(g2)[1] + pkg.g2_prepare(tau_g2)[1]
    openings, items = [], []
    for _ in range(args.distinct):
        coeffs = [rng.randrange(R) for _ in range(4)]
        z = rng.randrange(R)
        at = lambda x: sum(c * pow(x, e, R) for e, c in enumerate(coeffs)) % R
        y, ptau = at(z), at(tau)
        w = (ptau - y) * pow((tau - z) % R, -1, R) % R
        C, H = g1_of(ptau * s), g1_of(w * s)
        openings.append(C + H + z.to_bytes(32, "big") + y.to_bytes(32, "big"))
        items.append(g1_of((ptau - y + z * w) * s) + neg(H))
    d_key = torch.frombuffer(bytearray(key), dtype=torch.uint8).to(dev)
    d_recs = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    knob0 = pkg.kzg_params()
    lines, cells = [], []
    try:
        for n in sizes:
            reps = -(-n // args.distinct)
            d_open = torch.frombuffer(bytearray((b"".join(openings) * reps)[:192 * n]), dtype=torch.uint8).to(dev)
            d_items = torch.frombuffer(bytearray((b"".join(items) * reps)[:128 * n]), dtype=torch.uint8).to(dev)
            d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
            pkg.kzg_reserve(n, device=0)
            fns = {
                "exact": lambda: pkg.kzg_verify_batch_device(d_key.data_ptr(), d_open.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream),
                "rlc": lambda: pkg.kzg_verify_batch_device(d_key.data_ptr(), d_open.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream, flags=pkg.FLAG_RLC),
                "pairing": lambda: pkg.pairing_check_batch_shared_device(d_items.data_ptr(), 2, 0b11, d_recs.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream),
            }
            pkg.set_kzg_params(64)
            times = {name: [] for name in fns}
            s0 = pkg.kzg_state()
            for it in range(args.steps + 1):
                for name, fn in fns.items():
                    d_status.fill_(0xEE)
                    torch.cuda.synchronize(dev)
                    t = time.perf_counter()
                    fn()
                    torch.cuda.synchronize(dev)
                    if it:
                        times[name].append((time.perf_counter() - t) * 1e3)
                    assert bytes(d_status.cpu().numpy().tobytes()) == bytes([pkg.ACCEPT]) * n, name
            s1 = pkg.kzg_state()
            assert s1[0] - s0[0] == args.steps + 1 and s1[2] == s0[2] and s1[3] - s0[3] == args.steps + 1       # the weighted calls ran the joint check, no group failed
            m = {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}
            cells.append({"n": n, **{k: {"median_ms": round(v[0], 3), "min_ms": round(v[1], 3), "max_ms": round(v[2], 3)} for k, v in m.items()}})
            lines.append("n = %6d:  exact %9.3f ms (%.3f .. %.3f)   rlc %9.3f ms (%.3f .. %.3f)   pairing alone %9.3f ms (%.3f .. %.3f)   rlc / exact %.2f   exact / pairing alone %.2f"
                         % (n, *m["exact"], *m["rlc"], *m["pairing"], m["rlc"][0] / m["exact"][0], m["exact"][0] / m["pairing"][0]))
            print(lines[-1], flush=True)
    finally:
        pkg.set_kzg_params(knob0)
    head = ("bn254_kzg_verify_batch_device, exact and with BN254_FLAG_RLC honoured (bn254_set_kzg_params(64)), and bn254_pairing_check_batch_shared_device on the same openings "
            "restated as (F_i, -H_i) with F_i precomputed (the pairing alone); device-resident, one GPU (%s); the three alternating call by call, median of %d calls each "
            "(min .. max), each timed from the call to the status bytes on the device; valid openings (%d distinct, tiled)" % (torch.cuda.get_device_name(0), args.steps, args.distinct))
    with open(args.out, "w") as f:
        f.write(head + "\n\n" + "\n".join(lines) + "\n")
    print(json.dumps({"bench": "kzg_batch", "cells": cells}))


def main_fold(args):
    import hashlib
    import torch
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    from oracle import oracle as O
    O.build(); O.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sizes = [int(x) for x in args.sizes.split(",")]
    ks = [int(x) for x in args.digests.split(",")]
    dl = args.data_len
    rng = random.Random(0x18)
    s, tau = rng.randrange(2, R), rng.randrange(2, R)
    gen = O.g1_gen()
    memo = {}

    def g1_of(a):
        a %= R
        if a not in memo:
            memo[a] = bytes(64) if a == 0 else O.g1_mul(gen, a)
        return memo[a]

    be = lambda v: v.to_bytes(32, "big")
    st, key = pkg.kzg_key_prepare(g1_of(s), O.g2_gen(), O.g2_mul(O.g2_gen(), tau))
    assert st == pkg.ACCEPT
    # --distinct polynomials with their commitments; a record of k digests takes k of them at one point
    polys = [[rng.randrange(R) for _ in range(4)] for _ in range(args.distinct + max(ks))]
    at = lambda c, x: sum(a * pow(x, e, R) for e, a in enumerate(c)) % R
    ptau = [at(c, tau) for c in polys]
    commit = [g1_of(p * s) for p in ptau]

    def record(j, k, dl):
        z = rng.randrange(R)
        ys = [at(polys[j + i], z) for i in range(k)]
        data = bytes(rng.randrange(256) for _ in range(dl))
        digests = b"".join(commit[j + i] for i in range(k))
        g = int.from_bytes(hashlib.sha256(b"gamma" + be(z) + digests + b"".join(be(y) for y in ys) + data).digest(), "big") % R
        w = sum(pow(g, i, R) * (ptau[j + i] - ys[i]) for i in range(k)) % R * pow((tau - z) % R, -1, R) % R
        return digests + g1_of(w * s) + be(z) + b"".join(be(y) for y in ys) + data

    d_key = torch.frombuffer(bytearray(key), dtype=torch.uint8).to(dev)
    knob0 = pkg.kzg_params()
    lines, cells = [], []
    try:
        for n in sizes:
            reps = -(-n // args.distinct)
            openings = [record(j, 1, 0) for j in range(args.distinct)]      # one digest, no data: an opening
            d_open = torch.frombuffer(bytearray((b"".join(openings) * reps)[:192 * n]), dtype=torch.uint8).to(dev)
            d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
            pkg.kzg_reserve(n, device=0)
            med = {}
            for k in ks:
                rl = pkg.kzg_fold_len(k, dl)
                d_rec = torch.frombuffer(bytearray((b"".join(record(j, k, dl) for j in range(args.distinct)) * reps)[:rl * n]), dtype=torch.uint8).to(dev)
                pkg.kzg_fold_reserve(n, k, device=0)
                fns = {
                    "opening_exact": lambda: pkg.kzg_verify_batch_device(d_key.data_ptr(), d_open.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream),
                    "fold_exact": lambda: pkg.kzg_verify_folded_batch_device(d_key.data_ptr(), d_rec.data_ptr(), n, k, d_status.data_ptr(), data_len=dl, device=0, stream=stream.cuda_stream),
                    "opening_rlc": lambda: pkg.kzg_verify_batch_device(d_key.data_ptr(), d_open.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream, flags=pkg.FLAG_RLC),
                    "fold_rlc": lambda: pkg.kzg_verify_folded_batch_device(d_key.data_ptr(), d_rec.data_ptr(), n, k, d_status.data_ptr(), data_len=dl, device=0, stream=stream.cuda_stream,
                                                                         flags=pkg.FLAG_RLC),
                }
                pkg.set_kzg_params(64)
                times = {name: [] for name in fns}
                s0 = pkg.kzg_state()
                # the order of the four calls changes from round to round so that no entry always follows the same neighbour (a rotation would keep the neighbours: a call
                # right behind a short weighted call and one right behind a long exact call differ by about 0.1 ms at 65 536 records, whatever they run)
                names, perms = list(fns), ((0, 1, 2, 3), (0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1), (0, 2, 1, 3))
                for it in range(args.steps + 1):
                    for name in [names[q] for q in perms[it % len(perms)]]:
                        fn = fns[name]
                        d_status.fill_(0xEE)
                        torch.cuda.synchronize(dev)
                        t = time.perf_counter()
                        fn()
                        torch.cuda.synchronize(dev)
                        if it:
                            times[name].append((time.perf_counter() - t) * 1e3)
                        assert bytes(d_status.cpu().numpy().tobytes()) == bytes([pkg.ACCEPT]) * n, (name, k)
                s1 = pkg.kzg_state()
                assert s1[2] == s0[2] and s1[0] > s0[0] and s1[3] > s0[3]      # weighted and exact launches ran, no group failed
                m = {name: (statistics.median(v), min(v), max(v)) for name, v in times.items()}
                med[k] = m
                cells.append({"n": n, "digests": k, "data_len": dl, **{name: {"median_ms": round(v[0], 3), "min_ms": round(v[1], 3), "max_ms": round(v[2], 3)} for name, v in m.items()}})
                lines.append("n = %6d  k = %2d:  fold exact %9.3f ms (%.3f .. %.3f)   fold rlc %9.3f ms (%.3f .. %.3f)   |  openings exact %9.3f ms (%.3f .. %.3f)   openings rlc %9.3f ms "
                             "(%.3f .. %.3f)   |  fold / openings: exact %.3f  rlc %.3f   fold rlc / fold exact %.2f"
                             % (n, k, *m["fold_exact"], *m["fold_rlc"], *m["opening_exact"], *m["opening_rlc"], m["fold_exact"][0] / m["opening_exact"][0],
                                m["fold_rlc"][0] / m["opening_rlc"][0], m["fold_rlc"][0] / m["fold_exact"][0]))
                print(lines[-1], flush=True)
            if len(ks) > 1:
                lo, hi = min(ks), max(ks)
                lines.append("n = %6d:  per further digest (k = %d -> %d): exact %.3f ms = %.1f ns per record, rlc %.3f ms = %.1f ns per record"
                             % (n, lo, hi, (med[hi]["fold_exact"][0] - med[lo]["fold_exact"][0]) / (hi - lo), (med[hi]["fold_exact"][0] - med[lo]["fold_exact"][0]) / (hi - lo) / n * 1e6,
                                (med[hi]["fold_rlc"][0] - med[lo]["fold_rlc"][0]) / (hi - lo), (med[hi]["fold_rlc"][0] - med[lo]["fold_rlc"][0]) / (hi - lo) / n * 1e6))
                print(lines[-1], flush=True)
    finally:
        pkg.set_kzg_params(knob0)
    head = ("bn254_kzg_verify_folded_batch_device (batch-opening records of k digests, data_len %d), exact and with BN254_FLAG_RLC honoured (bn254_set_kzg_params(64)), alternating call "
            "by call with bn254_kzg_verify_batch_device on plain openings at the same n (the order of the four calls changes from round to round); device-resident, one GPU (%s); median of %d calls each (min .. max), each timed from the "
            "call to the status bytes on the device; valid records (%d distinct, tiled)" % (dl, torch.cuda.get_device_name(0), args.steps, args.distinct))
    with open(args.out, "w") as f:
        f.write(head + "\n\n" + "\n".join(lines) + "\n")
    print(json.dumps({"bench": "kzg_fold", "cells": cells}))


if __name__ == "__main__":
    main()
