#!/usr/bin/env python3
"""Static resources and instruction counts of every gfx950 kernel in a build of libbn254_verify_amd.so, one line per kernel:
VGPRs, AGPRs, spilled VGPRs, scratch bytes (the metadata notes of the code objects) and, from the disassembly, all instructions, VALU instructions,
v_mad_[iu]64_[iu]32, v_lshl_add_u64 and hazard nops.

  python tools/kernel_resources.py [LIB] [LABEL]                  # one build
  python tools/kernel_resources.py --compare LIB_A LIB_B          # A = parent form, B = candidate: both lines per kernel and the adoption rule

The adoption rule ("carry ride"): a kernel takes the candidate's form only if its spilled VGPRs and scratch bytes do not rise and its VALU
count falls."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "snark-bn254-verifier_amd", "libbn254_verify_amd.so")
FIELDS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("spill", ".vgpr_spill_count"), ("scratch", ".private_segment_fixed_size"))
RX = (("valu", re.compile(r"^v_")), ("mad64", re.compile(r"^v_mad_[iu]64_[iu]32\b")), ("lshl_add64", re.compile(r"^v_lshl_add_u64\b")), ("nop", re.compile(r"^s_nop\b")))


def demangled(sym):
    m = re.match(r"_ZN5bn254(\d+)(.*)", sym)       # bn254::name or bn254::name<bool>
    if not m:
        return sym
    n = int(m.group(1))
    name, rest = m.group(2)[:n], m.group(2)[n:]
    t = re.match(r"ILb([01])EE", rest)
    return name + ("<%s>" % ("true" if t.group(1) == "1" else "false") if t else "")


def kernels_of(lib):
    out = collections.OrderedDict()
    with tempfile.TemporaryDirectory() as wd:
        shutil.copy(lib, os.path.join(wd, "lib.so"))
        subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], stdout=subprocess.DEVNULL, cwd=wd)
        for co in sorted(f for f in os.listdir(wd) if "amdgcn" in f):
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(wd, co)], text=True)
            meta = {}
            for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                block = ".agpr_count:" + block
                sym = re.search(r"\.symbol:\s+(\S+)\.kd", block).group(1)
                meta[sym] = {k: int(re.search(re.escape(f) + r":\s+(\d+)", block).group(1)) for k, f in FIELDS}
            cur = None
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", os.path.join(wd, co)], text=True).splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = None
                    if m.group(1) in meta:
                        cur = dict(meta[m.group(1)], text=[])
                        out[demangled(m.group(1))] = cur
                    continue
                if cur is None or "//" not in line:
                    continue
                text = line.split("//", 1)[0].strip()
                if not text or text.startswith("s_code_end"):
                    continue
                cur["text"].append(text)
    for e in out.values():
        text = e.pop("text")
        while text and text[-1].startswith("s_nop"):     # alignment padding behind the kernel's last instruction
            text.pop()
        e["instr"] = len(text)
        for k, rx in RX:
            e[k] = sum(1 for t in text if rx.match(t))
    return out


COLS = ("vgpr", "agpr", "spill", "scratch", "instr", "valu", "mad64", "lshl_add64", "nop")


def line(label, name, e, extra=""):
    return "%-9s %-34s " % (label, name) + " ".join("%8d" % e[c] for c in COLS) + extra


def main():
    head = "# %-7s %-34s " % ("build", "kernel") + " ".join("%8s" % c for c in COLS)
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        a, b = kernels_of(sys.argv[2]), kernels_of(sys.argv[3])
        print(head + "  verdict")
        for name in sorted(b):
            if name not in a:
                print(line("ride", name, b[name], "  (new)"))
                continue
            x, y = a[name], b[name]
            same = all(x[c] == y[c] for c in COLS)
            ok = y["spill"] <= x["spill"] and y["scratch"] <= x["scratch"] and y["valu"] < x["valu"]
            print(line("parent", name, x))
            print(line("ride", name, y, "  " + ("same" if same else "ADOPT %+d valu" % (y["valu"] - x["valu"]) if ok else "KEEP parent (%+d valu, %+d spill, %+d scratch)" % (y["valu"] - x["valu"], y["spill"] - x["spill"], y["scratch"] - x["scratch"]))))
        return
    lib = sys.argv[1] if len(sys.argv) > 1 else LIB
    label = sys.argv[2] if len(sys.argv) > 2 else "build"
    print(head)
    for name, e in sorted(kernels_of(lib).items()):
        print(line(label, name, e))


if __name__ == "__main__":
    main()
