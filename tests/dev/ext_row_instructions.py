#!/usr/bin/env python3
"""Development aid (CPU): the instructions per ROW of the anchored extension's row loops, read out of the built gfx950 code object - the figures
DESIGN 7i-9 derives its expectation for the per-lane motif from.  For every instantiation of mtr_k_ext_lanes<UB> (the dense partial genotype:
the motif wave-uniform, rows compiled without a cut for U == UB and masked rows otherwise) and of mtr_k_ptc_ext<UB> (the call at catalogue scale:
masked rows, the motif per lane) the kernel is disassembled with llvm-objdump and every backward branch is taken as a loop: its first and last
instruction's index, its length, and how many of its instructions are VALU (v_*), SALU (s_*) and v_mov.  The row loop is the long loop that ends
BEFORE the early-exit test of a word's edge (the shorter of each pair that shares a start); a kernel with two such pairs holds the uncut rows
second.  Divide by UB for instructions per cell.  Prints one line per kernel."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_kernel_resources as tkr  # noqa: E402


def loops(txt, name):
    m = re.search(r"^([0-9a-f]+) <" + re.escape(name) + r">:\n(.*?)(?=^[0-9a-f]+ <_Z|\Z)", txt, re.S | re.M)
    base = int(m.group(1), 16)
    raw = [l for l in m.group(2).splitlines() if re.search(r"//\s*[0-9A-F]{8,}:", l)]
    ins = [(int(re.search(r"//\s*([0-9A-F]{8,}):", l).group(1), 16), l.strip().split("//")[0].strip()) for l in raw]
    addr = {a: i for i, (a, _) in enumerate(ins)}
    out = []
    for i, l in enumerate(raw):
        if not l.strip().startswith(("s_cbranch", "s_branch")):
            continue
        t = re.search(r"<" + re.escape(name) + r"\+0x([0-9a-f]+)>", l)
        if t and base + int(t.group(1), 16) in addr and addr[base + int(t.group(1), 16)] <= i:
            first = addr[base + int(t.group(1), 16)]
            body = [x[1] for x in ins[first:i + 1]]
            out.append({"first": first, "last": i, "instructions": len(body), "valu": sum(b.startswith("v_") for b in body),
                        "salu": sum(b.startswith("s_") for b in body), "v_mov": sum(b.startswith("v_mov") for b in body)})
    return len(ins), out


def main():
    with tempfile.TemporaryDirectory() as d:
        import pathlib

        co = tkr._code_object(pathlib.Path(d))
        objdump = os.path.join(os.path.dirname(tkr.READELF), "llvm-objdump")
        txt = subprocess.run([objdump, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    for name in sorted(set(re.findall(r"<(_Z\d+mtr_k_(?:ext_lanes|ptc_ext)ILi\d+EEv\d+\w+Args)>:", txt))):
        total, found = loops(txt, name)
        print(name, total, "instructions;", "loops:", [f for f in found if f["instructions"] > 100])


if __name__ == "__main__":
    main()
