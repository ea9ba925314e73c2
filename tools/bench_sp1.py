#!/usr/bin/env python3
"""The SP1 entries (public values hashed on the device by k_sp1_public_inputs, then the unchanged pipeline) against the raw entries on the same proofs with the
rows vkey_hash | digest computed beforehand.
  python tools/bench_sp1.py [--sizes 4096,65536,1048576] [--value-bytes 96,1024,4096] [--steps 3] [--no-host] [--no-plonk]
Rows: Groth16 device entry at every size x value length; Groth16 host entry at every size with the first value length and at 65 536 proofs with the others;
PlonK device and host entries at 65 536 proofs (the SP1 fixtures, cycled).  Every proof of a row carries the same values (the hash costs the same whatever the
bytes); the proofs are made for the first value length, so the other lengths verify as REJECT -- the same pipeline work -- and the status bytes of the two
runs are compared either way.  Every call is timed on its own to its status bytes (device entries: on the device; host entries: in host memory).  One JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536,1048576")
    ap.add_argument("--value-bytes", type=str, default="96,1024,4096")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-plonk", action="store_true")
    args = ap.parse_args()
    import ctypes as C
    import torch
    import sp1_data as S
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

    L = pkg.lib()
    host_args = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    L.bn254_sp1_groth16_verify_batch.argtypes = host_args
    L.bn254_sp1_plonk_verify_batch.argtypes = host_args

    def host_pair(raw_fn, sp1_fn, handle, proofs, stride, inputs, vkh, vstride, values, n):
        """The two host entries called directly on buffers packed beforehand: the timed region is the C call (staging copies included), not Python packing."""
        pv, offs = pkg.sp1_pack_values(values)
        st = (C.c_uint8 * n)()

        def raw():
            assert raw_fn(handle, proofs, stride, inputs, 2, n, st, 0, 0) == 0
            return bytes(st)

        def sp1():
            assert sp1_fn(handle, proofs, stride, vkh, vstride, pv, C.cast(offs, C.c_void_p), n, st, 0, 0) == 0
            return bytes(st)
        return timed(raw) + timed(sp1)

    def put(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def row(proto, entry, n, vb, raw_ms, raw_st, sp1_ms, sp1_st):
        assert raw_st == sp1_st, (proto, entry, n, vb)
        rows.append({"proto": proto, "entry": entry, "batch": n, "value_bytes": vb, "raw_ms": round(raw_ms, 3), "sp1_ms": round(sp1_ms, 3),
                     "ratio": round(sp1_ms / raw_ms, 4), "accept": sum(1 for x in sp1_st if x == pkg.ACCEPT)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    sizes = [int(x) for x in args.sizes.split(",")]
    vbs = [int(x) for x in args.value_bytes.split(",")]
    big = max(sizes)
    vkh = (12345).to_bytes(32, "big")
    blob = {vb: bytes((7 * k + vb) & 0xFF for k in range(vb)) for vb in vbs}
    t0 = time.perf_counter()
    vk, proofs = pkg.synth_groth16_for_inputs(0x5B1BE, 2, (vkh + S.digest(blob[vbs[0]])) * big, threads=16)
    print("made %d proofs in %.1f s" % (big, time.perf_counter() - t0), file=sys.stderr, flush=True)
    pvk = pkg.PreparedVk(vk)
    pvk.reserve(big, 0)
    d_proofs = put(proofs)
    d_vkh = put(vkh)
    for vb in vbs:
        d_rows = put((vkh + S.digest(blob[vb])) * big)
        d_pv = put(blob[vb] * big)
        d_off = torch.arange(0, (big + 1) * vb, vb, dtype=torch.int64, device=dev)
        for n in sizes:
            ds = torch.zeros(n, dtype=torch.uint8, device=dev)

            def raw():
                ds.fill_(0xEE)
                pvk.verify_batch_device(d_proofs.data_ptr(), d_rows.data_ptr(), ds.data_ptr(), n, 256, 2, 0, st.cuda_stream)
                st.synchronize()
                return bytes(ds.cpu().numpy().tobytes())

            def sp1():
                ds.fill_(0xEE)
                pvk.verify_sp1_batch_device(d_proofs.data_ptr(), d_vkh.data_ptr(), d_pv.data_ptr(), n * vb, d_off.data_ptr(), ds.data_ptr(), n, vkey_stride=0,
                                            stream=st.cuda_stream)
                st.synchronize()
                return bytes(ds.cpu().numpy().tobytes())
            r_ms, r_st = timed(raw)
            s_ms, s_st = timed(sp1)
            row("groth16", "device", n, vb, r_ms, r_st, s_ms, s_st)
            del ds
        del d_rows, d_pv, d_off
        if not args.no_host:
            for n in (sizes if vb == vbs[0] else [x for x in sizes if x == 65536]):
                values = [blob[vb]] * n
                inputs = (vkh + S.digest(blob[vb])) * n
                p = proofs[:256 * n]
                r_ms, r_st, s_ms, s_st = host_pair(L.bn254_groth16_verify_batch, L.bn254_sp1_groth16_verify_batch, pvk.handle, p, 256, inputs, vkh, 0, values, n)
                row("groth16", "host", n, vb, r_ms, r_st, s_ms, s_st)
    pvk.close()
    if not args.no_plonk:
        ppvk = pkg.PreparedPlonkVk(open(os.path.join(ROOT, "tests", "golden", "plonk_vk.bin"), "rb").read())
        items = [S.fixture(name, "plonk") for name in S.NAMES]
        n = 65536
        sel = [items[i % 4] for i in range(n)]
        pb = b"".join(it[1] for it in sel)
        vkhs = [it[2][:32] for it in sel]
        values = [it[4] for it in sel]
        inputs = b"".join(it[2] for it in sel)
        pv = b"".join(values)
        offs = [0]
        for v in values:
            offs.append(offs[-1] + len(v))
        dp, di, dh, dv = put(pb), put(inputs), put(b"".join(vkhs)), put(pv)
        do = torch.tensor(offs, dtype=torch.int64, device=dev)
        ds = torch.zeros(n, dtype=torch.uint8, device=dev)

        def praw():
            ppvk.verify_batch_device(dp.data_ptr(), di.data_ptr(), ds.data_ptr(), n, 904, 2, 0, st.cuda_stream)
            return bytes(ds.cpu().numpy().tobytes())

        def psp1():
            ppvk.verify_sp1_batch_device(dp.data_ptr(), dh.data_ptr(), dv.data_ptr(), len(pv), do.data_ptr(), ds.data_ptr(), n, stream=st.cuda_stream)
            return bytes(ds.cpu().numpy().tobytes())
        r_ms, r_st = timed(praw)
        s_ms, s_st = timed(psp1)
        row("plonk", "device", n, "fixtures", r_ms, r_st, s_ms, s_st)
        if not args.no_host:
            r_ms, r_st, s_ms, s_st = host_pair(L.bn254_plonk_verify_batch_flags, L.bn254_sp1_plonk_verify_batch, ppvk._h, pb, 904, inputs, b"".join(vkhs), 32, values, n)
            row("plonk", "host", n, "fixtures", r_ms, r_st, s_ms, s_st)
        ppvk.close()
    print(json.dumps({"bench": "sp1", "steps": args.steps, "rows": rows}))


if __name__ == "__main__":
    main()
