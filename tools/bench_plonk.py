#!/usr/bin/env python3
"""PlonK batch verification rate (BASELINE configs[3]: batch 4096, SP1 circuit, 2 public inputs) on one MI355X: bench.plonk_config as a
stand-alone command (`bench.py --full` carries the same measurement in its `configs` block).  Prints one JSON line.

--distinct: the same timed loop on a generated workload in which every proof is different (bn254_synth_plonk) instead of the four SP1 fixtures repeated: the
fixtures make every lane of a wavefront gather the same four entries per window of the key's tables, a real batch scatters its reads over them.  The invalid
proofs are made as the fixture workload makes them (a flipped public-input bit at every 8th position), so the two runs differ in nothing but the proofs.
--shape NPUB,NQCP,LOG2 picks the key shape of the generated workload; shapes other than the SP1 one (2 inputs, 1 commitment: 904-byte proofs) run the
device-resident loop alone (exact and, from 8192 proofs, BN254_FLAG_RLC), since bench.plonk_config is laid out for 904-byte proofs with two inputs."""
import argparse, importlib, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DISTINCT_SEED = 0xB2540D15


def distinct_workload(pkg, shape, batch):
    """bench.plonk_workload's batch with generated proofs: all valid and distinct, then one flipped public-input bit at every 8th position (the same draws)."""
    n_public, n_qcp, log2 = shape
    vk, pb, ib, _ = pkg.synth_plonk(DISTINCT_SEED, n_public, n_qcp, log2, batch, invalid_every=0, threads=16)
    plen, ilen = 808 + 96 * n_qcp, 32 * n_public
    rng = random.Random(4)
    ib = bytearray(ib)
    if ilen:
        for i in range(7, batch, 8):
            ib[ilen * i + rng.randrange(ilen)] ^= 1 << rng.randrange(8)
    ib = bytes(ib)
    return vk, pb, ib, [pb[plen * i:plen * (i + 1)] for i in range(batch)], [ib[ilen * i:ilen * (i + 1)] for i in range(batch)]


def shape_config(pkg, shape, batch, steps, warmup, cpu_sample):
    """The device-resident loop of bench.plonk_config for a key of any shape: proofs, inputs and status bytes in HBM, `steps` calls timed after `warmup`."""
    import torch
    from oracle import oracle as O
    n_public, n_qcp, log2 = shape
    vk, pb, ib, proofs, inputs = distinct_workload(pkg, shape, batch)
    plen = 808 + 96 * n_qcp
    pvk = pkg.PreparedPlonkVk(vk)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_p = torch.frombuffer(bytearray(pb), dtype=torch.uint8).to(dev); d_q = torch.frombuffer(bytearray(ib or b"\0"), dtype=torch.uint8).to(dev)
    d_st = torch.full((batch,), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    out = {}
    for name, flags in (("exact", 0),) + ((("rlc", pkg.FLAG_RLC),) if batch >= 8192 else ()):
        def resident():
            pvk.verify_batch_device(d_p.data_ptr(), d_q.data_ptr(), d_st.data_ptr(), batch, proof_stride=plen, n_public=n_public, device=dev.index, stream=stream.cuda_stream, flags=flags)
        for _ in range(max(1, warmup)):
            resident()
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        for _ in range(steps):
            resident()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t
        st = bytes(d_st.cpu().numpy().tobytes())
        bad = batch // 8 if n_public else 0
        assert st.count(bytes([pkg.ACCEPT])) == batch - bad, "PlonK: %d ACCEPT of %d" % (st.count(bytes([pkg.ACCEPT])), batch)
        m = min(cpu_sample, batch)
        assert st[:m] == bytes(O.plonk_verify(proofs[i], vk, [inputs[i][32 * j:32 * j + 32] for j in range(n_public)]) for i in range(m)), "PlonK: GPU statuses differ from the oracle"
        out[name] = {"value": batch * steps / dt, "unit": "proofs/s", "ms_per_step": dt * 1e3 / steps}
    pvk.close()
    return {"workload": "PlonK batch %d, %d-byte generated proofs, all distinct, %d public inputs, %d commitments, 2^%d rows, %s; resident in HBM"
                        % (batch, plen, n_public, n_qcp, log2, "1/8 invalid" if n_public else "all valid"),
            "value": out["exact"]["value"], "unit": "proofs/s", "ms_per_step": out["exact"]["ms_per_step"], "steps": steps, "batch": batch,
            "rlc_mode": {"unit": "proofs/s", "exact": out["exact"]["value"], "rlc": out["rlc"]["value"], "speedup": out["rlc"]["value"] / out["exact"]["value"],
                         "ms_per_step": out["rlc"]["ms_per_step"]} if "rlc" in out else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-sample", type=int, default=64)
    ap.add_argument("--no-in-flight", action="store_true", help="skip the two / four calls in flight measurement (kernel traces: one call at a time only)")
    ap.add_argument("--distinct", action="store_true", help="a generated workload of all-distinct proofs instead of the four SP1 fixtures repeated")
    ap.add_argument("--shape", default="2,1,26", help="NPUB,NQCP,LOG2 of the generated key (with --distinct); default: the SP1 shape")
    args = ap.parse_args()
    shape = tuple(int(x) for x in args.shape.split(","))
    if len(shape) != 3:
        ap.error("--shape takes NPUB,NQCP,LOG2")
    if shape != (2, 1, 26) and not args.distinct:
        ap.error("--shape needs --distinct: the fixtures have one shape")
    import bench
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    data = "reference fixtures + mutations"
    if args.distinct:
        data = "generated proofs (bn254_synth_plonk, seed %#x, shape %s), all distinct, + the same mutations" % (DISTINCT_SEED, args.shape)
        if shape[:2] == (2, 1):
            bench.plonk_workload = lambda batch: distinct_workload(pkg, shape, batch)      # the workload, and nothing else, of bench.plonk_config
    bench.plonk_config(pkg, args.batch, 2, 1, 0, in_flight=False)      # warms the GPU: the peak probe reads low on idle clocks
    bench.measure_valu_peak(pkg)
    if args.distinct and shape[:2] != (2, 1):
        r = shape_config(pkg, shape, args.batch, args.steps, args.warmup, args.cpu_sample)
    else:
        r = bench.plonk_config(pkg, args.batch, args.steps, args.warmup, args.cpu_sample, in_flight=args.batch <= 8192 and not args.no_in_flight)
        if args.distinct:
            r["workload"] = r["workload"].replace("the reference's fixtures + mutations", "generated, all distinct, 2^%d rows" % shape[2])
    r.update({"metric": "PlonK verifies/sec at batch=%d (proofs resident in HBM; `host_buffers` beside it)" % args.batch, "n_gpus": 1, "warmup": args.warmup,
              "higher_is_better": True, "dtype": "int64", "data": data, "config": {"workload": r["workload"]}})
    print(json.dumps(r))


if __name__ == "__main__":
    main()
