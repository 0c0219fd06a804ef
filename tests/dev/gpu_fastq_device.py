#!/usr/bin/env python3
"""Development aid: what reading FASTQ on the device costs on the headline shape (10 000 reads of ~2 kb, synth "headline2k").  The same
reads are written as FASTQ and as single-line FASTA, and three routes to the resident batch are timed, alternating, after a warm-up:
  upload_fastq_device   the FASTQ bytes in a GPU tensor -> the batch (mtr_upload_fastq_device + mtr_fasta_index): a line table, no compaction;
  upload_fasta_device   the FASTA bytes in a GPU tensor -> the batch (mtr_upload_fasta_device + mtr_fasta_index);
  host_route            the FASTQ bytes back to the host (.cpu()), stripped to the reads with numpy, Engine.upload.
Each route ends in a synchronise of the device work, so each is timed twice over the same calls: by the host clock around the call, and by
a pair of HIP events on torch's current stream around it (the library waits for that stream and is done before it returns, so the pair
brackets its work).  Then the batch is run after a FASTQ and after a FASTA upload and the wire bytes are compared.  Prints one JSON line;
--out FILE writes it there as well.  Kernel time: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_fastq_device.py"""
import argparse
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

ACGT = np.frombuffer(b"ACGT", np.uint8)
LUT = np.full(256, 255, np.uint8)
for _c, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    LUT[_c] = _v


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def strip_fastq(raw: np.ndarray):
    """the reads of a well-formed four-line FASTQ file as codes, with numpy: the sequence lines are lines 1, 5, 9, ..."""
    lf = np.flatnonzero(raw == 10)
    starts, ends = lf[0::4] + 1, lf[1::4]
    return [LUT[raw[s:e]] for s, e in zip(starts.tolist(), ends.tolist())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    named = synth.make_reads("headline2k", a.reads)
    seqs = [(str(rid).encode(), ACGT[codes].tobytes()) for rid, codes in named]
    fastq = b"".join(b"@" + i + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in seqs)
    fasta = b"".join(b">" + i + b"\n" + s + b"\n" for i, s in seqs)
    dev = torch.device("cuda", 0)
    eng = mtr_amd.Engine(0)
    d_fastq = torch.from_numpy(np.frombuffer(fastq, np.uint8).copy()).to(dev)
    d_fasta = torch.from_numpy(np.frombuffer(fasta, np.uint8).copy()).to(dev)
    torch.cuda.synchronize()

    def host_route():
        eng.upload(strip_fastq(d_fastq.cpu().numpy()))

    routes = {"upload_fastq_device": lambda: eng.upload_fastq_device(d_fastq), "upload_fasta_device": lambda: eng.upload_fasta_device(d_fasta),
              "host_route": host_route}
    clock, events = {k: [] for k in routes}, {k: [] for k in routes}
    for rep in range(a.warmup + a.reps):
        for name, fn in routes.items():                         # alternating: the routes share whatever else the machine is doing
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                clock[name].append((time.perf_counter() - t) * 1e3)
                events[name].append(e0.elapsed_time(e1))
    out = {"reads": len(named), "bases": int(sum(len(s) for _, s in seqs)), "fastq_bytes": len(fastq), "fasta_bytes": len(fasta)}
    for name in routes:
        out[name + "_ms"] = {"host_clock": stats(clock[name]), "hip_events": stats(events[name])}

    fq = eng.upload_fastq_device(d_fastq)
    eng.run()
    got = eng.fetch_packed()[0]
    fa = eng.upload_fasta_device(d_fasta)
    eng.run()
    out["identical_wire_bytes"] = got == eng.fetch_packed()[0] and fq.end == "eof" and fq.ids == fa.ids and len(fq.ids) == len(named)
    eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if out["identical_wire_bytes"] else 1


if __name__ == "__main__":
    sys.exit(main())
