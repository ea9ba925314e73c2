#!/usr/bin/env python3
"""Times of the KZG batch (bn254_kzg_verify_batch_device) on one GPU: device-resident openings at n in {4096, 65536, 262144}, the exact entry and the entry with
BN254_FLAG_RLC honoured (bn254_set_kzg_params(64)) ALTERNATING call by call in one session, and beside them bn254_pairing_check_batch_shared_device on the same openings
restated as items (F_i, -H_i) with F_i precomputed on the host -- the pairing alone, the floor of the exact entry.
  python tools/bench_kzg.py [--sizes 4096,65536,262144] [--steps 5] [--out profiles/r17_kzg_batch.txt]
The openings are --distinct (default 512) valid openings of random cubic polynomials under a key with known trapdoors, tiled to n: the kernels' work does not depend on
the values, and a valid batch never reaches the fallback of the weighted path (its best case; a failed group adds the per-opening check of its wavefront).  Every call
is timed on its own from the call to the status bytes on the device, after one warm-up call and a reservation; the median of --steps calls is reported with its
min .. max.  Writes the table to --out and prints one JSON line."""
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
    ap.add_argument("--sizes", type=str, default="4096,65536,262144")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r17_kzg_batch.txt"))
    args = ap.parse_args()
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


if __name__ == "__main__":
    main()
