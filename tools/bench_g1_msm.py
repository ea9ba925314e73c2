#!/usr/bin/env python3
"""Times of the batch G1 multi-scalar multiplication (bn254_g1_msm_batch_device) on one GPU: device-resident items at n in {4096, 65536, 262144} for the shapes
(1,0,0), (2,0,0), (8,0,0), (16,0,0), (0,2,0), (2,1,0), (0,0,2), (0,0,16), (2,1,16), the shapes ALTERNATING call by call in one session, and beside them as orientation
rows bn254_kzg_verify_batch_device (exact) and bn254_pairing_check_batch_shared_device on the same openings restated as items (F_i, -H_i) -- their difference is the
(2,1,0) walk behind another loader.
  python tools/bench_g1_msm.py [--sizes 4096,65536,262144] [--steps 5] [--out profiles/r19_g1_msm.txt]
The items are --distinct (default 512) valid items of random multiples of G1 with full-width scalars, tiled to n: the kernels' work does not depend on the values.  Every
call is timed on its own from the call to the bytes on the device, after one warm-up call and a reservation; the median of --steps calls is reported with its min .. max.
Writes the table to --out and prints one JSON line."""
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
SHAPES = ((1, 0, 0), (2, 0, 0), (8, 0, 0), (16, 0, 0), (0, 2, 0), (2, 1, 0), (0, 0, 2), (0, 0, 16), (2, 1, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536,262144")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r19_g1_msm.txt"))
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    from oracle import oracle as O
    O.build(); O.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sizes = [int(x) for x in args.sizes.split(",")]
    rng = random.Random(0x19)
    gen = O.g1_gen()
    pool = [O.g1_mul(gen, rng.randrange(2, R)) for _ in range(64)]
    be = lambda x: int(x).to_bytes(32, "big")
    neg = lambda p: p if p == bytes(64) else p[:32] + be((P - int.from_bytes(p[32:], "big")) % P)
    st, bases = pkg.g1_bases_prepare(b"".join(pool[:16]), device=0)
    assert st == pkg.ACCEPT

    def item(v, u, s):
        return b"".join(rng.choice(pool) + be(rng.randrange(R)) for _ in range(v)) + b"".join(rng.choice(pool) for _ in range(u)) + b"".join(be(rng.randrange(R)) for _ in range(s))

    distinct = {sh: b"".join(item(*sh) for _ in range(args.distinct)) for sh in SHAPES}
    # the orientation rows: valid KZG openings and the items (F_i, -H_i) the pairing alone checks
    s_, tau = rng.randrange(2, R), rng.randrange(2, R)
    g1_of = lambda a: bytes(64) if a % R == 0 else O.g1_mul(gen, a % R)
    g2, tau_g2 = O.g2_gen(), O.g2_mul(O.g2_gen(), tau)
    st, key = pkg.kzg_key_prepare(g1_of(s_), g2, tau_g2)
    assert st == pkg.ACCEPT
    recs = pkg.g2_prepare(g2)[1] + pkg.g2_prepare(tau_g2)[1]
    openings, pitems = [], []
    for _ in range(args.distinct):
        coeffs = [rng.randrange(R) for _ in range(4)]
        z = rng.randrange(R)
        at = lambda x: sum(c * pow(x, e, R) for e, c in enumerate(coeffs)) % R
        y, ptau = at(z), at(tau)
        w = (ptau - y) * pow((tau - z) % R, -1, R) % R
        C, H = g1_of(ptau * s_), g1_of(w * s_)
        openings.append(C + H + be(z) + be(y))
        pitems.append(g1_of((ptau - y + z * w) * s_) + neg(H))
    d_key = torch.frombuffer(bytearray(key), dtype=torch.uint8).to(dev)
    d_recs = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    lines = ["# tools/bench_g1_msm.py: device-resident items, median of %d alternating calls (min .. max), ms per call" % args.steps]
    cells = []
    try:
        for n in sizes:
            reps = -(-n // args.distinct)
            d_out = torch.full((64 * n,), 0xEE, dtype=torch.uint8, device=dev)
            d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
            d_items = {}
            fns = {}
            for sh in SHAPES:
                ilen = pkg.g1_msm_item_len(*sh)
                d_items[sh] = torch.frombuffer(bytearray((distinct[sh] * reps)[:ilen * n]), dtype=torch.uint8).to(dev)
                pkg.g1_msm_reserve(n, *sh, device=0)
                fns["g1_msm %d,%d,%d" % sh] = (lambda sh=sh: pkg.g1_msm_batch_device(d_items[sh].data_ptr(), *sh, n, d_out.data_ptr(), d_status.data_ptr(),
                                                                                      bases=bases if sh[2] else None, device=0, stream=stream.cuda_stream))
            d_open = torch.frombuffer(bytearray((b"".join(openings) * reps)[:192 * n]), dtype=torch.uint8).to(dev)
            d_pit = torch.frombuffer(bytearray((b"".join(pitems) * reps)[:128 * n]), dtype=torch.uint8).to(dev)
            pkg.kzg_reserve(n, device=0)
            fns["kzg exact"] = lambda: pkg.kzg_verify_batch_device(d_key.data_ptr(), d_open.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream)
            fns["pairing alone"] = lambda: pkg.pairing_check_batch_shared_device(d_pit.data_ptr(), 2, 0b11, d_recs.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream)
            times = {k: [] for k in fns}
            for k, f in fns.items():      # warm-up
                f(); stream.synchronize()
            assert bytes(d_status.cpu().numpy().tobytes()) == bytes([pkg.ACCEPT]) * n
            for step in range(args.steps):
                order = list(fns)
                order = order[step % len(order):] + order[:step % len(order)]      # the neighbour in the round changes from round to round
                for k in order:
                    stream.synchronize()
                    t0 = time.perf_counter()
                    fns[k]()
                    stream.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3)
            lines.append("n = %d" % n)
            for k, ts in times.items():
                med = statistics.median(ts)
                lines.append("  %-18s %9.3f  (%.3f .. %.3f)" % (k, med, min(ts), max(ts)))
                cells.append({"n": n, "row": k, "median_ms": med, "min_ms": min(ts), "max_ms": max(ts)})
            diff = statistics.median(times["kzg exact"]) - statistics.median(times["pairing alone"])
            lines.append("  kzg exact - pairing alone = %.3f ms (the (2,1,0) walk behind the KZG loader); g1_msm 2,1,0 = %.3f ms" % (diff, statistics.median(times["g1_msm 2,1,0"])))
            var1, sh2 = statistics.median(times["g1_msm 2,0,0"]) - statistics.median(times["g1_msm 1,0,0"]), statistics.median(times["g1_msm 0,0,16"]) / 16
            lines.append("  one further variable term = %.3f ms; one shared term (the (0,0,16) row / 16) = %.3f ms" % (var1, sh2))
    finally:
        bases.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    print(json.dumps({"bench": "g1_msm", "cells": cells}))


if __name__ == "__main__":
    main()
