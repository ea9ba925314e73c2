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
                form --form names (plan, lane or coop); a cell gives both medians, each one's min .. max and the ratio
  --rlc SHAPES  times bn254_pairing_check_batch_flags_device with BN254_FLAG_RLC honoured (bn254_set_pairing_rlc_params(64)) against bn254_pairing_check_batch_shared_device
                on the same device-resident, ALL-VALID packed items, alternating call by call in one session; SHAPES as for --shared, mask 0 being the all-variable item,
                e.g. 2:0x3,4:0xe,8:0xff,1:0,4:0,8:0.  An item is valid because its positions cancel in twos -- (P, Q) beside (-P, Q), a shared Q standing at both
                positions, and where a variable position has to cancel against a shared one its G2 bytes are that point in every item; a lone position holds the identity
                of G1.  --fail-per-group adds, per shape, a run in which item 5 of every group of 64 is invalid: the worst case of the fallback"""
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
    ap.add_argument("--rlc", type=str, default="", help="K:MASK[,K:MASK...]: time the flags entry with BN254_FLAG_RLC against the shared entry on all-valid items")
    ap.add_argument("--fail-per-group", action="store_true", help="--rlc: also time batches with one invalid item in every group of 64")
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
    rlc_shapes = [(int(t.split(":")[0]), int(t.split(":")[1], 0)) for t in args.rlc.split(",") if t]
    if rlc_shapes:
        return bench_rlc(args, pkg, torch, np, dev, stream, sizes, rlc_shapes, timed_pair)
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


def bench_rlc(args, pkg, torch, np, dev, stream, sizes, shapes, timed_pair):
    P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    if args.form == "lane":
        pkg.set_pairing_params(0)
    elif args.form == "coop":
        pkg.set_pairing_params(30720)
    knob0 = pkg.pairing_rlc_params()
    pkg.set_pairing_rlc_params(64)
    rows, lines = [], []

    def negated(pts):
        """(x, y) -> (x, p - y) for an array of 64-byte points"""
        out = pts.copy()
        for i in range(len(pts)):
            y = int.from_bytes(pts[i, 32:64].tobytes(), "big")
            out[i, 32:64] = np.frombuffer(((P - y) % P).to_bytes(32, "big"), dtype=np.uint8)
        return out

    for n in sizes:
        _, proofs, _, _ = pkg.synth_groth16(0xB2549000, 2, n, invalid_every=0, agree=True, threads=16)
        rec = np.frombuffer(proofs, dtype=np.uint8).reshape(n, 256)
        a, b = rec[:, 0:64], rec[:, 64:192]
        neg = {}
        pkg.pairing_reserve(n, device=0)
        for k, mask in shapes:
            sh = [j for j in range(k) if (mask >> j) & 1]
            var = [j for j in range(k) if not (mask >> j) & 1]
            # positions cancel in twos within a kind; a leftover of each kind cancels across the kinds (the variable one carries the shared point's bytes); a lone
            # leftover holds the identity of G1
            twos = [(sh[i], sh[i + 1]) for i in range(0, len(sh) - 1, 2)] + [(var[i], var[i + 1]) for i in range(0, len(var) - 1, 2)]
            left = ([sh[-1]] if len(sh) % 2 else []) + ([var[-1]] if len(var) % 2 else [])
            if len(left) == 2:
                twos.append((left[0], left[1])); left = []
            pts, g2s = {}, {}
            for t, (x, y) in enumerate(twos):
                pj = np.roll(a, -7 * t, axis=0)
                if t not in neg:
                    neg[t] = negated(pj)
                pts[x], pts[y] = pj, neg[t]
                fixed = x in sh or y in sh
                qj = np.repeat(b[13 * t % n:13 * t % n + 1], n, axis=0) if fixed else np.roll(b, -13 * t, axis=0)
                g2s[x] = g2s[y] = qj
            for x in left:
                pts[x] = np.zeros((n, 64), dtype=np.uint8)
                g2s[x] = np.repeat(b[:1], n, axis=0) if x in sh else b
            recs, cols = [], []
            for j in range(k):
                cols.append(pts[j])
                if j in sh:
                    st, r = pkg.g2_prepare(g2s[j][0].tobytes())
                    assert st == pkg.ACCEPT
                    recs.append(r)
                else:
                    cols.append(g2s[j])
            packed = np.ascontiguousarray(np.concatenate(cols, axis=1))
            d_prep = torch.frombuffer(bytearray(b"".join(recs) if recs else bytes(4)), dtype=torch.uint8).to(dev)
            prep_ptr = d_prep.data_ptr() if recs else 0
            cases = [("valid", packed)]
            if args.fail_per_group:
                bad = packed.copy()
                first = twos[0][0] if twos else None
                if first is not None:
                    off = sum(64 if (mask >> j) & 1 else 192 for j in range(first))
                    bad[5::64, off:off + 64] = np.roll(a, -3, axis=0)[5::64]      # another valid point: the item's positions no longer cancel
                    cases.append(("one invalid item per group", bad))
            for label, items in cases:
                d_items = torch.from_numpy(items).to(dev)
                d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
                d_st2 = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
                s0 = pkg.pairing_rlc_state()
                res = timed_pair({
                    "rlc": lambda: pkg.pairing_check_batch_shared_device(d_items.data_ptr(), k, mask, prep_ptr, n, d_st.data_ptr(), device=0, stream=stream.cuda_stream, flags=pkg.FLAG_RLC),
                    "exact": lambda: pkg.pairing_check_batch_shared_device(d_items.data_ptr(), k, mask, prep_ptr, n, d_st2.data_ptr(), device=0, stream=stream.cuda_stream)})
                s1 = pkg.pairing_rlc_state()
                got, ref = bytes(d_st.cpu().numpy().tobytes()), bytes(d_st2.cpu().numpy().tobytes())
                assert got == ref, "the two entries disagree"
                want_bad = 0 if label == "valid" else len(range(5, n, 64))
                assert got.count(bytes([pkg.ACCEPT])) == n - want_bad and got.count(bytes([pkg.REJECT])) == want_bad, {x: got.count(bytes([x])) for x in set(got)}
                assert s1[0] - s0[0] == args.steps + 1 and s1[3] == s0[3], "the flag was not honoured"
                (rm, rlo, rhi), (em, elo, ehi) = res["rlc"], res["exact"]
                rows.append({"n": n, "n_pairs": k, "shared_mask": mask, "case": label, "form": args.form, "rlc_ms": round(rm, 3), "rlc_min": round(rlo, 3), "rlc_max": round(rhi, 3),
                             "exact_ms": round(em, 3), "exact_min": round(elo, 3), "exact_max": round(ehi, 3), "failed_groups_per_call": (s1[2] - s0[2]) // (args.steps + 1)})
                lines.append("n = %6d   n_pairs = %d  mask = 0x%02x  %-26s  RLC %8.3f ms (%.3f .. %.3f)   exact %8.3f ms (%.3f .. %.3f)   RLC / exact %.2f"
                             % (n, k, mask, label + ":", rm, rlo, rhi, em, elo, ehi, rm / em))
    pkg.set_pairing_rlc_params(knob0)
    head = ["bn254_pairing_check_batch_flags_device with BN254_FLAG_RLC honoured (rlc_min 64) against bn254_pairing_check_batch_shared_device on the same all-valid packed items, "
            "device-resident, one GPU (%s); the two entries alternating call by call, median of %d calls each (min .. max) after a warm-up call, each timed from the call to "
            "the status bytes on the device; form: %s" % (torch.cuda.get_device_name(0), args.steps, args.form), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print(json.dumps({"bench": "pairing_batch_rlc", "rows": rows}))


if __name__ == "__main__":
    main()
