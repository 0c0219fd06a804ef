#!/usr/bin/env python3
"""Development aid: what the -a alignments of the report cost on the headline batch (10 000 reads of ~2 kb, synth "headline2k"), by two
routes that both start from the same Engine.report_tensors():
  A  fields / units to the host -> mtr_record structs (numpy, vectorised) -> mtr_alignments (the clock stops when it returns: turning
     its paths into text rows is NOT counted)
  B  Engine.report_alignment_tensors() (mtr_report_alignments_device: tasks, alignment and rendered rows on the device)
Each repetition runs the batch again first (untimed): a run clears the context's chains and alignments, so every timed call of B
makes them anew.  One warm-up repetition, then --reps timed ones by the host clock.  Prints one JSON line; --out FILE writes it too.
Kernel times: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_report_align.py --reps 3"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the first Engine: one HIP runtime serves both)
import numpy as np  # noqa: E402

import mtr_amd  # noqa: E402
from mtr_amd import synth  # noqa: E402

REC = C.sizeof(mtr_amd.CRecord)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def route_a(eng, rep):
    read = np.ascontiguousarray(rep.read.cpu().numpy(), np.int32)
    fields, unit_off, units = rep.fields.cpu().numpy(), rep.unit_off.cpu().numpy(), rep.units.cpu().numpy()
    R = len(read)
    recs = np.zeros((max(R, 1), REC), np.uint8)
    recs[:R, :56] = np.ascontiguousarray(fields, np.int32).view(np.uint8).reshape(R, 56)
    ulen = np.diff(unit_off)
    recs[np.repeat(np.arange(R), ulen), 56 + np.arange(len(units)) - np.repeat(unit_off[:-1], ulen)] = units
    po, pf, pe = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
    eng._check(eng.lib.mtr_alignments(eng.h, R, read.ctypes.data_as(C.POINTER(C.c_int32)), recs.ctypes.data, C.byref(po), C.byref(pf), C.byref(pe)),
               "mtr_alignments")
    columns = int(pf[R])
    for p in (po, pf, pe):
        mtr_amd._libc.free(C.cast(p, C.c_void_p))
    return columns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    reads = [c for _, c in synth.make_reads("headline2k", a.reads, synth.CONFIGS["headline2k"][4])]
    eng = mtr_amd.Engine()
    eng.upload(reads)
    a_ms, b_ms = [], []
    for _ in range(a.reps + 1):
        eng.run()
        rep = eng.report_tensors()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cols_a = route_a(eng, rep)
        a_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        al = eng.report_alignment_tensors()
        torch.cuda.synchronize()
        b_ms.append((time.perf_counter() - t0) * 1e3)
        assert cols_a == al.ops.numel()
    out = {"reads": a.reads, "repeats": int(rep.counts.sum()), "columns": int(al.ops.numel()),
           "route_a_host_records_mtr_alignments_ms": stats(a_ms[1:]), "route_b_report_alignment_tensors_ms": stats(b_ms[1:])}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
