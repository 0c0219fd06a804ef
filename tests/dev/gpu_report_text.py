#!/usr/bin/env python3
"""Development aid: what mTR's stdout costs a library caller on the headline batch (10 000 reads of ~2 kb, synth "headline2k"), plain and
with -a's alignments, by two routes to the same host bytes:
  A  the columns' route: Engine.report_tensors() (plus report_alignment_tensors()), their copies to the host, mtr_amd.format_report
  B  Engine.report_bytes() (mtr_report_text_device: sized, laid out and written on the device; one copy of the finished text)
Each repetition runs the batch again first (untimed): a run clears the context's chains and alignments, so every timed call makes them
anew, in both routes.  The routes alternate; one warm-up repetition, then --reps timed ones by the host clock (both routes end in a
device-to-host copy).  The bytes of the two routes are compared every time.  Prints one JSON line; --out FILE writes it too.
Kernel times: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_report_text.py --reps 2 --new-only"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the first Engine: one HIP runtime serves both)

import mtr_amd  # noqa: E402
from mtr_amd import synth  # noqa: E402


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def route_a(eng, ids, lens, alignments):
    rep = eng.report_tensors()
    al = eng.report_alignment_tensors() if alignments else None
    return mtr_amd.format_report(ids, lens, rep, alignments=al)           # (format_report makes the .cpu() copies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--new-only", action="store_true", help="route B alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    reads = [c for _, c in synth.make_reads("headline2k", a.reads, synth.CONFIGS["headline2k"][4])]
    ids, lens = [str(i) for i in range(len(reads))], [len(r) for r in reads]
    eng = mtr_amd.Engine()
    eng.upload(reads)
    out = {"reads": a.reads}
    for alignments in (False, True):
        a_ms, b_ms, nbytes = [], [], 0
        for _ in range(a.reps + 1):
            want = None
            if not a.new_only:
                eng.run()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                want = route_a(eng, ids, lens, alignments)
                a_ms.append((time.perf_counter() - t0) * 1e3)
            eng.run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = eng.report_bytes(ids, alignments=alignments)
            b_ms.append((time.perf_counter() - t0) * 1e3)
            assert want is None or got == want
            nbytes = len(got)
        mode = "alignments" if alignments else "plain"
        out[mode] = {"bytes": nbytes, "route_b_report_bytes_ms": stats(b_ms[1:])}
        if a_ms:
            out[mode]["route_a_columns_format_report_ms"] = stats(a_ms[1:])
    out["repeats"] = int(eng.report_tensors().counts.sum())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
