#!/usr/bin/env python3
"""BN254_FLAG_COMPRESSED_PROOFS against the raw layout: the same proofs, gnark-compressed (128 bytes, decompressed on the device by k_g16_decompress) and raw
(256 bytes).
  python tools/bench_compressed.py [--sizes 4096,65536,1048576] [--wide 1024:4096] [--steps 3] [--no-host] [--no-rlc]
Rows: the device entry (inputs resident in HBM) at every size with 2 public inputs and at the --wide (inputs:proofs) shape; the host-buffer entry and
BN254_FLAG_RLC (device entry, the default threshold: honoured at this size) at the largest size.  Every call is timed on its own (from the call to the status
bytes on the device; the host entry: to the status bytes in host memory) and its status bytes are checked against the raw run's.  One JSON line."""
import argparse
import importlib
import json
import statistics
import sys
import os
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536,1048576")
    ap.add_argument("--wide", type=str, default="1024:4096")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-rlc", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    rows = []

    def timed(fn):
        times, out = [], None
        for it in range(args.steps + 1):
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize(dev)
            if it:
                times.append(time.perf_counter() - t)
        return statistics.median(times) * 1e3, out

    def workload(n_public, n):
        vk, proofs, inputs, _ = pkg.synth_groth16(0xB2547000 + n_public, n_public, n, invalid_every=0, agree=True, threads=32)
        t = time.perf_counter()
        recs = b"".join(pkg.compress_proof(proofs[256 * i:256 * (i + 1)]) for i in range(n))
        print("compressed %d proofs on the host in %.1f s (single thread, Python loop)" % (n, time.perf_counter() - t), file=sys.stderr, flush=True)
        return vk, proofs, inputs, recs

    def device_row(pvk, proofs, recs, inputs, n_public, n, flags, entry):
        dp = torch.frombuffer(bytearray(proofs[:256 * n]), dtype=torch.uint8).to(dev)
        dc = torch.frombuffer(bytearray(recs[:128 * n]), dtype=torch.uint8).to(dev)
        di = torch.frombuffer(bytearray(inputs[:32 * n_public * n]) if n_public else bytearray(1), dtype=torch.uint8).to(dev)
        ds = torch.zeros(n, dtype=torch.uint8, device=dev)

        def run(ptr, stride, compressed):
            def f():
                ds.fill_(0xEE)
                pvk.verify_batch_device(ptr, di.data_ptr(), ds.data_ptr(), n, stride, n_public, 0, st.cuda_stream, flags=flags, compressed=compressed)
                st.synchronize()
                return bytes(ds.cpu().numpy().tobytes())
            return f
        raw_ms, raw_st = timed(run(dp.data_ptr(), 256, False))
        cmp_ms, cmp_st = timed(run(dc.data_ptr(), 128, True))
        assert raw_st == cmp_st and set(raw_st) == {pkg.ACCEPT}, (entry, n_public, n)
        del dp, dc, di, ds
        return {"entry": entry, "n_public": n_public, "batch": n, "raw_ms": round(raw_ms, 3), "compressed_ms": round(cmp_ms, 3),
                "raw_proofs_per_s": round(n / raw_ms * 1e3), "compressed_proofs_per_s": round(n / cmp_ms * 1e3), "ratio": round(cmp_ms / raw_ms, 4)}

    sizes = [int(x) for x in args.sizes.split(",")]
    big = max(sizes)
    vk, proofs, inputs, recs = workload(2, big)
    pvk = pkg.PreparedVk(vk)
    pvk.reserve(big, 0)
    for n in sizes:
        rows.append(device_row(pvk, proofs, recs, inputs, 2, n, 0, "device"))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    if not args.no_host:
        raw_ms, raw_st = timed(lambda: pvk.verify_batch(proofs, inputs, big, 256, 2))
        cmp_ms, cmp_st = timed(lambda: pvk.verify_batch(recs, inputs, big, 128, 2, compressed=True))
        assert raw_st == cmp_st and set(raw_st) == {pkg.ACCEPT}
        rows.append({"entry": "host", "n_public": 2, "batch": big, "raw_ms": round(raw_ms, 3), "compressed_ms": round(cmp_ms, 3),
                     "raw_proofs_per_s": round(big / raw_ms * 1e3), "compressed_proofs_per_s": round(big / cmp_ms * 1e3), "ratio": round(cmp_ms / raw_ms, 4)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    if not args.no_rlc:
        rows.append(device_row(pvk, proofs, recs, inputs, 2, big, pkg.FLAG_RLC, "device_rlc"))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    pvk.close()
    if args.wide:
        wp, wn = (int(x) for x in args.wide.split(":"))
        vk, proofs, inputs, recs = workload(wp, wn)
        pvk = pkg.PreparedVk(vk)
        pvk.reserve(wn, 0)
        rows.append(device_row(pvk, proofs, recs, inputs, wp, wn, 0, "device"))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        pvk.close()
    print(json.dumps({"bench": "compressed", "steps": args.steps, "rows": rows}))


if __name__ == "__main__":
    main()
