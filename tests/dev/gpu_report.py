#!/usr/bin/env python3
"""Development aid: what the device report costs on the headline batch (10 000 reads of ~2 kb, synth "headline2k").
After one run, times Engine.report_tensors() (mtr_report_device: the chain kernel mtr_k_chain + the column kernel mtr_k_report_pack,
plus the count / offset copies around them) against fetch_packed() + the host chain (mtrh_chain of libmtr_host.so, one call per read
through ctypes) by the host clock.  Each repetition runs the batch again first (untimed): a run clears the context's chains, so
every timed report_tensors() makes them anew.  Prints one JSON line; --out FILE writes it there as well.
Kernel time: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_report.py"""
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


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    host = C.CDLL(os.path.join(ROOT, "mtr_amd", "host", "libmtr_host.so"))
    host.mtrh_chain.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    host.mtrh_chain.restype = C.c_int
    reads = [c for _, c in synth.make_reads("headline2k", a.reads, synth.CONFIGS["headline2k"][4])]
    eng = mtr_amd.Engine()
    eng.upload(reads)
    eng.run()
    dev_ms, host_ms = [], []
    for _ in range(a.reps + 1):
        eng.run()
        t0 = time.perf_counter()
        rep = eng.report_tensors()
        torch.cuda.synchronize()
        dev_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        blob, counts = eng.fetch_packed()
        buf = np.frombuffer(blob, np.uint8)
        off, n_rep = 0, 0
        chain = np.zeros(int(counts.max()) if len(counts) else 1, np.int32)
        for c in counts:
            recs = np.zeros((max(int(c), 1), 3), np.uint64)
            for t in range(int(c)):
                per = int(buf[off + 12: off + 16].view(np.int32)[0])
                recs[t, 0] = buf.ctypes.data + off
                off += 56 + ((per + 3) & ~3) + 4 * per
            n_rep += host.mtrh_chain(recs.ctypes.data, int(c), chain.ctypes.data)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        assert n_rep == int(rep.counts.sum())
    out = {"reads": a.reads, "repeats": int(rep.counts.sum()), "report_tensors_ms": stats(dev_ms[1:]),
           "fetch_packed_plus_host_chain_ms": stats(host_ms[1:])}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
