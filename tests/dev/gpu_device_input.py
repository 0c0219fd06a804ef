#!/usr/bin/env python3
"""Development aid: what reads already in device memory save on the headline batch (10 000 reads of ~2 kb, synth "headline2k").
Times three uploads of the same batch - host codes (mtr_upload_batch: packed on the calling thread, copied), device ASCII text and
device code text (mtr_upload_batch_device: the packing kernel mtr_k_pack_text) - then run + fetch after each, and checks that all
three give the same wire bytes.  Each upload is timed by the host clock around the call (it returns after the device work) and by
HIP events on torch's stream around it.  Prints one JSON line; --out FILE writes it there as well.
Kernel time: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_device_input.py"""
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


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--run-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    reads = [c for _, c in synth.make_reads("headline2k", a.reads)]
    bases, offs, lens = mtr_amd._flatten(reads)
    dev = torch.device("cuda", 0)
    t_codes = torch.from_numpy(bases).to(dev)
    t_ascii = torch.from_numpy(np.frombuffer(b"ACGT", np.uint8)[bases]).to(dev)
    torch.cuda.synchronize()
    eng = mtr_amd.Engine(0)
    variants = {"host_codes": lambda: eng.upload_flat(bases, offs, lens),
                "device_ascii": lambda: eng.upload_device(t_ascii, offs, lens),
                "device_codes": lambda: eng.upload_device(t_codes, offs, lens, codes=True)}
    out = {"reads": len(reads), "bases": int(lens.sum()), "text_bytes": int(bases.nbytes),
           "packed_bytes": int((lens.astype(np.int64) // 16 + 4).sum() * 4)}
    blobs = {}
    for name, up in variants.items():
        for _ in range(a.warmup):
            up()
        wall, ev = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t = time.perf_counter()
            up()
            wall.append((time.perf_counter() - t) * 1e3)
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        run = []
        for _ in range(a.run_reps):
            up()
            t = time.perf_counter()
            eng.run()
            blob, _ = eng.fetch_packed()
            run.append((time.perf_counter() - t) * 1e3)
        blobs[name] = blob
        out[name] = {"upload_ms_wall": stats(wall), "upload_ms_events": stats(ev), "run_fetch_ms_wall": stats(run)}
    out["identical_wire_bytes"] = len(set(blobs.values())) == 1
    eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if out["identical_wire_bytes"] else 1


if __name__ == "__main__":
    sys.exit(main())
