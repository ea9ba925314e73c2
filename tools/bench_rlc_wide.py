#!/usr/bin/env python3
"""BN254_FLAG_RLC against the exact path for keys with more than 8 public inputs (group scalars, bn254_rlc.h): proofs/s per width and batch size.
  python tools/bench_rlc_wide.py [--widths 1024,40] [--sizes 4096,16384,65536] [--steps 3] [--invalid-every 0]
Inputs resident in HBM (the device entry); every call is timed on its own (from the first launch to the statuses on the device) and its status bytes are
checked against the generator's.  The RLC rows run with bn254_set_rlc_params(64, 0, -1) (the flag honoured at every size, no adaptive bypass); the
defaults are restored at the end.  One JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=str, default="1024,40")
    ap.add_argument("--sizes", type=str, default="4096,16384,65536")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--invalid-every", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    dev = torch.device("cuda:0")
    rows = []
    pkg.set_rlc_params(min_batch=64, adaptive=0)
    try:
        for n_public in [int(x) for x in args.widths.split(",")]:
            for n in [int(x) for x in args.sizes.split(",")]:
                vk, proofs, inputs, exp = pkg.synth_groth16(0xB2546000 + n_public, n_public, n, invalid_every=args.invalid_every, agree=True, threads=16)
                if args.invalid_every:
                    # the generator places its invalid proofs periodically and the groups are index classes: shuffle for the placement of a real batch
                    perm = np.random.default_rng(n).permutation(n)
                    proofs = np.frombuffer(proofs, dtype=np.uint8).reshape(n, 256)[perm].tobytes()
                    inputs = np.frombuffer(inputs, dtype=np.uint8).reshape(n, 32 * n_public)[perm].tobytes()
                    exp = np.frombuffer(exp, dtype=np.uint8)[perm].tobytes()
                pvk = pkg.PreparedVk(vk)
                pvk.reserve(n, 0)
                dp = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).to(dev)
                di = torch.frombuffer(bytearray(inputs), dtype=torch.uint8).to(dev)
                ds = torch.zeros(n, dtype=torch.uint8, device=dev)
                st = torch.cuda.current_stream(dev)
                row = {"n_public": n_public, "batch": n, "invalid_every": args.invalid_every}
                for name, flags in (("exact", 0), ("rlc", pkg.FLAG_RLC)):
                    times = []
                    for it in range(args.steps + 1):
                        ds.fill_(0xEE)
                        torch.cuda.synchronize(dev)
                        t = time.perf_counter()
                        pvk.verify_batch_device(dp.data_ptr(), di.data_ptr(), ds.data_ptr(), n, 256, n_public, 0, st.cuda_stream, flags=flags)
                        torch.cuda.synchronize(dev)
                        dt = time.perf_counter() - t
                        assert bytes(ds.cpu().numpy().tobytes()) == exp, (name, n_public, n, it)
                        if it:
                            times.append(dt)
                    ms = statistics.median(times) * 1e3
                    row[name + "_ms"] = round(ms, 3)
                    row[name + "_proofs_per_s"] = round(n / ms * 1e3)
                row["speedup"] = round(row["exact_ms"] / row["rlc_ms"], 3)
                row["fallback_share"] = pvk.rlc_state()[0]
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                pvk.close()
                del dp, di, ds
    finally:
        pkg.set_rlc_params(min_batch=200000, adaptive=1)
    print(json.dumps({"bench": "rlc_wide", "group_log2": int(os.environ.get("BN254_RLC_GROUP_LOG2", "5")), "steps": args.steps, "rows": rows}))


if __name__ == "__main__":
    main()
