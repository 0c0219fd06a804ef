#!/usr/bin/env python3
"""Development aid: what the motif catalogue costs on the headline batch (10 000 reads of ~2 kb, synth "headline2k").  Per repetition the
batch is run again (untimed): a run clears the context's chains and catalogue, so every timed call makes them anew.  Then, by the host
clock around calls that end in a stream synchronise:
  report_first_ms   the first mtr_report_device call after the run (dst == NULL): the chains - the code every report call shares
  report_pack_ms    the second one, into preallocated columns: the pack
  motifs_first_ms   the first mtr_report_motifs_device call (dst == NULL): the chains exist, so it holds the catalogue's own work alone -
                    unit_motif per repeat, the table, the scans, the aggregation
  motifs_copy_ms    the second one, into preallocated columns: eleven device-to-device copies
One warm-up repetition, then --reps timed ones; medians.  Prints one JSON line with R and G; --out FILE writes it too.
Kernel times: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_report_motifs.py --reps 2"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the first Engine: one HIP runtime serves both)

import mtr_amd  # noqa: E402
from mtr_amd import synth  # noqa: E402


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def timed(fn):
    t0 = time.perf_counter()
    st = fn()
    ms = (time.perf_counter() - t0) * 1e3
    assert st == 0, st
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    reads = [c for _, c in synth.make_reads("headline2k", a.reads, synth.CONFIGS["headline2k"][4])]
    eng = mtr_amd.Engine()
    eng.upload(reads)
    eng.run()
    rep, mot = eng.report_tensors(), eng.report_motif_tensors()               # the sizes of this batch, and the columns every repetition writes
    R, U, G, M = rep.read.numel(), rep.units.numel(), mot.g_first.numel(), mot.motifs.numel()
    ptr = lambda t: t.data_ptr() if t.numel() else None                       # noqa: E731
    rdst = mtr_amd.CReportDst(*[ptr(t) for t in rep[1:]], R, U)
    mdst = mtr_amd.CReportMotifDst(*[ptr(t) for t in mot], R, G, M)
    counts = np.zeros(len(reads), np.int32)
    n1, n2, n3 = C.c_int64(), C.c_int64(), C.c_int64()
    lib, h = eng.lib, eng.h
    ms = {k: [] for k in ("report_first_ms", "report_pack_ms", "motifs_first_ms", "motifs_copy_ms")}
    for _ in range(a.reps + 1):
        eng.run()
        torch.cuda.synchronize()
        ms["report_first_ms"].append(timed(lambda: lib.mtr_report_device(h, None, counts.ctypes.data, C.byref(n1), C.byref(n2))))
        ms["report_pack_ms"].append(timed(lambda: lib.mtr_report_device(h, C.byref(rdst), counts.ctypes.data, C.byref(n1), C.byref(n2))))
        ms["motifs_first_ms"].append(timed(lambda: lib.mtr_report_motifs_device(h, None, C.byref(n1), C.byref(n2), C.byref(n3))))
        ms["motifs_copy_ms"].append(timed(lambda: lib.mtr_report_motifs_device(h, C.byref(mdst), C.byref(n1), C.byref(n2), C.byref(n3))))
        assert (n1.value, n2.value, n3.value) == (R, G, M)
    out = {"reads": a.reads, "repeats": R, "groups": G, "motif_bytes": M, "unit_bytes": U}
    out.update({k: stats(v[1:]) for k, v in ms.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
