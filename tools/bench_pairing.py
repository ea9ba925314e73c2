#!/usr/bin/env python3
"""Rates of the batch pairing product (bn254_pairing_check_batch_device) on one GPU: device-resident items, n in {4096, 65536} x n_pairs in {1, 2, 3, 4, 8}, items/s per
cell, and in the same session the exact Groth16 rate (bn254_groth16_verify_batch_device, 2 public inputs) at the same n for orientation.
  python tools/bench_pairing.py [--sizes 4096,65536] [--pairs 1,2,3,4,8] [--steps 5] [--out profiles/r14_pairing_batch.txt]
The items are made of the A (G1) and B (G2) points of a synthetic Groth16 workload, pair j of item i being (A[i + 7 j], B[i + 13 j]) (indices modulo n): distinct valid
points, so every item runs its loops to the end and is REJECT (checked).  Every call is timed on its own from the call to the status bytes on the device, after one
warm-up call and a reservation; the median of --steps calls is reported.  Writes the table to --out and prints one JSON line.
  --form plan   the form the library chooses (bn254_set_pairing_params as it stands; the default)
  --form lane   bn254_set_pairing_params(0): the one-item-per-lane kernels at every size
  --form coop   bn254_set_pairing_params(30720): the cooperative twelve-lane kernel wherever it can run (n <= 30 720)
  --form both   both, ALTERNATING call by call inside every cell (lane, coop, lane, coop, ...), so that a drift of the machine meets both alike: the lane form of the
                same session is the reference of every cooperative figure; the cell also gives the spread (min .. max) of each form's calls
  --shared SHAPES   times bn254_pairing_check_batch_shared_device instead: SHAPES is a comma-separated list of K:MASK (or MASK alone, for every pair count of --pairs
                that holds it), e.g. 2:0x3,4:0xe,8:0xff,8:0xaa.  The G2 point of a shared position j is B[13 j] for every item, prepared once (bn254_g2_prepare); the
                shared entry on the PACKED items and the all-variable entry on the EXPANDED items (the same points) run ALTERNATING call by call in one session, in the
                form --form names (plan, lane or coop); a cell gives both medians, each one's min .. max and the ratio"""
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
    ap.add_argument("--sizes", type=str, default="4096,65536")
    ap.add_argument("--pairs", type=str, default="1,2,3,4,8")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r14_pairing_batch.txt"))
    ap.add_argument("--form", choices=("plan", "lane", "coop", "both"), default="plan")
    ap.add_argument("--shared", type=str, default="", help="K:MASK[,K:MASK...]: time the shared entry against the all-variable entry on the expanded items")
    ap.add_argument("--no-groth16", action="store_true", help="skip the Groth16 batch timed for orientation")
    args = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("snark-bn254-verifier_amd")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sizes = [int(x) for x in args.sizes.split(",")]
    pairs = [int(x) for x in args.pairs.split(",")]

    def timed(fn):
        times = []
        for it in range(args.steps + 1):
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if it:
                times.append(time.perf_counter() - t)
        return statistics.median(times) * 1e3

    COOP_MAX = 30720
    knob0 = pkg.pairing_params()

    def timed_both(fn):
        """lane and cooperative calls alternating; -> {form: (median, min, max)} in ms"""
        times = {"lane": [], "coop": []}
        for it in range(args.steps + 1):
            for form, knob in (("lane", 0), ("coop", COOP_MAX)):
                pkg.set_pairing_params(knob)
                torch.cuda.synchronize(dev)
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                if it:
                    times[form].append((time.perf_counter() - t) * 1e3)
        pkg.set_pairing_params(knob0)
        return {f: (statistics.median(v), min(v), max(v)) for f, v in times.items()}

    def timed_pair(fns):
        """the calls of fns (name -> callable) alternating; -> {name: (median, min, max)} in ms"""
        times = {name: [] for name in fns}
        for it in range(args.steps + 1):
            for name, fn in fns.items():
                torch.cuda.synchronize(dev)
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                if it:
                    times[name].append((time.perf_counter() - t) * 1e3)
        return {f: (statistics.median(v), min(v), max(v)) for f, v in times.items()}

    shapes = []
    for tok in [t for t in args.shared.split(",") if t]:
        if ":" in tok:
            shapes.append((int(tok.split(":")[0]), int(tok.split(":")[1], 0)))
        else:
            shapes += [(k, int(tok, 0)) for k in pairs if int(tok, 0) >> k == 0]
    if shapes and args.form == "both":
        ap.error("--shared compares the two ENTRIES in one form: --form plan, lane or coop")
    if args.form == "lane":
        pkg.set_pairing_params(0)
    elif args.form == "coop":
        pkg.set_pairing_params(COOP_MAX)
    rows, lines = [], []
    for n in sizes:
        vk, proofs, inputs, expected = pkg.synth_groth16(0xB2549000, 2, n, invalid_every=0, agree=True, threads=16)
        rec = np.frombuffer(proofs, dtype=np.uint8).reshape(n, 256)
        a, b = rec[:, 0:64], rec[:, 64:192]
        d_status = torch.zeros(n, dtype=torch.uint8, device=dev)
        g16_ms = None
        if not args.no_groth16:
            pvk = pkg.PreparedVk(vk, pkg.VK_REFERENCE)
            d_proofs = torch.from_numpy(rec.copy()).to(dev)
            d_inputs = torch.frombuffer(bytearray(inputs), dtype=torch.uint8).to(dev)
            pvk.reserve(n, 0)

            def g16():
                pvk.verify_batch_device(d_proofs.data_ptr(), d_inputs.data_ptr(), d_status.data_ptr(), n, 256, 2, 0, stream.cuda_stream)

            g16_ms = timed(g16)
            assert bytes(d_status.cpu().numpy().tobytes()) == expected
            lines.append("n = %d   exact Groth16 (2 inputs, device entry): %.3f ms, %.0f proofs/s" % (n, g16_ms, n / g16_ms * 1e3))
        pkg.pairing_reserve(n, device=0)
        for k, mask in shapes:
            expanded = np.empty((n, 192 * k), dtype=np.uint8)
            packed, recs = [], []
            for j in range(k):
                pj = np.roll(a, -7 * j, axis=0)
                qj = np.roll(b, -13 * j, axis=0)
                if (mask >> j) & 1:
                    qj = np.repeat(qj[:1], n, axis=0)                    # the point of position j, for every item
                    st, r = pkg.g2_prepare(qj[0].tobytes())
                    assert st == pkg.ACCEPT
                    recs.append(r)
                    packed.append(pj)
                else:
                    packed += [pj, qj]
                expanded[:, 192 * j:192 * j + 64] = pj
                expanded[:, 192 * j + 64:192 * j + 192] = qj
            d_exp = torch.from_numpy(expanded).to(dev)
            d_packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(packed, axis=1))).to(dev)
            d_prep = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(dev)
            d_st2 = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
            d_status.fill_(0xEE)
            res = timed_pair({
                "shared": lambda: pkg.pairing_check_batch_shared_device(d_packed.data_ptr(), k, mask, d_prep.data_ptr(), n, d_status.data_ptr(), device=0, stream=stream.cuda_stream),
                "variable": lambda: pkg.pairing_check_batch_device(d_exp.data_ptr(), k, n, d_st2.data_ptr(), device=0, stream=stream.cuda_stream)})
            got, ref = bytes(d_status.cpu().numpy().tobytes()), bytes(d_st2.cpu().numpy().tobytes())
            assert got == ref == bytes([pkg.REJECT]) * n, "unexpected status bytes: %r / %r" % ({x: got.count(bytes([x])) for x in set(got)}, {x: ref.count(bytes([x])) for x in set(ref)})
            (sm, slo, shi), (vm, vlo, vhi) = res["shared"], res["variable"]
            rows.append({"n": n, "n_pairs": k, "shared_mask": mask, "form": args.form, "shared_ms": round(sm, 3), "shared_min": round(slo, 3), "shared_max": round(shi, 3),
                         "variable_ms": round(vm, 3), "variable_min": round(vlo, 3), "variable_max": round(vhi, 3)})
            lines.append("n = %6d   n_pairs = %d  mask = 0x%02x:  shared %8.3f ms (%.3f .. %.3f)   all-variable %8.3f ms (%.3f .. %.3f)   shared / all-variable %.2f"
                         % (n, k, mask, sm, slo, shi, vm, vlo, vhi, sm / vm))
        for k in ([] if shapes else pairs):
            items = np.empty((n, 192 * k), dtype=np.uint8)
            for j in range(k):
                items[:, 192 * j:192 * j + 64] = np.roll(a, -7 * j, axis=0)
                items[:, 192 * j + 64:192 * j + 192] = np.roll(b, -13 * j, axis=0)
            d_items = torch.from_numpy(items).to(dev)
            d_status.fill_(0xEE)

            def run():
                pkg.pairing_check_batch_device(d_items.data_ptr(), k, n, d_status.data_ptr(), device=0, stream=stream.cuda_stream)

            if args.form == "both" and n <= COOP_MAX:
                both = timed_both(run)
                got = bytes(d_status.cpu().numpy().tobytes())
                assert got == bytes([pkg.REJECT]) * n, "unexpected status bytes: %r" % {s: got.count(bytes([s])) for s in set(got)}
                (lm, llo, lhi), (cm, clo, chi) = both["lane"], both["coop"]
                rows.append({"n": n, "n_pairs": k, "lane_ms": round(lm, 3), "lane_min": round(llo, 3), "lane_max": round(lhi, 3), "coop_ms": round(cm, 3), "coop_min": round(clo, 3),
                             "coop_max": round(chi, 3)})
                lines.append("n = %6d   n_pairs = %d:  lane %8.3f ms (%.3f .. %.3f)   coop %8.3f ms (%.3f .. %.3f)   coop / lane %.2f" % (n, k, lm, llo, lhi, cm, clo, chi, cm / lm))
                continue
            ms = timed(run)
            got = bytes(d_status.cpu().numpy().tobytes())
            assert got == bytes([pkg.REJECT]) * n, "unexpected status bytes: %r" % {s: got.count(bytes([s])) for s in set(got)}
            rows.append({"n": n, "n_pairs": k, "form": args.form, "ms": round(ms, 3), "items_per_s": round(n / ms * 1e3), "pairs_per_s": round(n * k / ms * 1e3),
                         "groth16_ms": round(g16_ms, 3) if g16_ms else None})
            lines.append("n = %d   n_pairs = %d: %.3f ms, %.0f items/s, %.0f pairs/s%s" % (n, k, ms, n / ms * 1e3, n * k / ms * 1e3,
                                                                                        ", %.2f x the Groth16 batch's time" % (ms / g16_ms) if g16_ms else ""))
    pkg.set_pairing_params(knob0)
    if shapes:
        head = ["bn254_pairing_check_batch_shared_device on packed items against bn254_pairing_check_batch_device on the expanded items (the same points), device-resident, one GPU "
                "(%s); the two entries alternating call by call, median of %d calls each (min .. max), each timed from the call to the status bytes on the device; form: %s"
                % (torch.cuda.get_device_name(0), args.steps, args.form), ""]
        with open(args.out, "w") as f:
            f.write("\n".join(head + lines) + "\n")
        print(json.dumps({"bench": "pairing_batch_shared", "rows": rows}))
        return
    head = ["bn254_pairing_check_batch_device, device-resident items, one GPU (%s); median of %d calls per cell, each timed from the call to the status bytes on the device; "
            "form: %s" % (torch.cuda.get_device_name(0), args.steps, "lane and cooperative alternating call by call (median, min .. max)" if args.form == "both" else args.form), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print(json.dumps({"bench": "pairing_batch", "rows": rows}))


if __name__ == "__main__":
    main()
