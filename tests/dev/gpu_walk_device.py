#!/usr/bin/env python3
"""Development aid: what walking a FASTA file in device memory batch by batch costs against one call on the whole file.  The file is
100 000 headline-shaped reads (synth "headline2k", ~2 kb each) written as single-line records, about 206 MB.  It times
  whole   one upload_fasta_device of all the bytes (mtr_upload_fasta_device: more_follows = 0, the path before the walk existed);
  walk    Engine.walk_fasta_device with windows of --window-mib (24 MiB, the command line's chunk): the summed time of its uploads
          (mtr_upload_fasta_device_window), per call as well, and the bytes parsed twice - each window's open record is parsed again
          by the next;
by the host clock around the calls (each returns after the device work), and reports for both the peak of the parser's buffers in
the context, computed from the sizes as mtr_abi.hip sizes them (tile columns 28 B a tile of 4096 B, header columns 20 B a record,
compacted text, offsets, lengths, IDs), and by how much the device's free memory fell over the case (that holds the resident batch
too).  Checks that the walk's reads are the whole file's.  Prints one JSON line; --out FILE writes it there as well.
Kernel time: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_walk_device.py"""
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

TILE = mtr_amd.FASTA_TILE_BYTES


def fasta_bytes(named, width):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts = []
    for rid, codes in named:
        s = acgt[codes].tobytes()
        body = s if not width else b"\n".join(s[i:i + width] for i in range(0, len(s), width))
        parts.append(b">" + str(rid).encode() + b"\n" + body + b"\n")
    return b"".join(parts)


def parser_bytes(n_bytes, f, open_record=0):
    """the parser's buffers for a call on n_bytes that returned f (open_record: 1 if a header behind the reads was seen)"""
    tiles, heads, n = (n_bytes + TILE - 1) // TILE, len(f.ids) + open_record, len(f.ids)
    return (7 * tiles + 2) * 4 + 3 * heads * 4 + (heads + 1) * 8 + int(f.lens.sum()) + 16 + n * 12 + sum(len(i) for i in f.ids) + 16


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--width", type=int, default=0, help="wrap the sequence lines at this many columns (0: one line a record)")
    ap.add_argument("--window-mib", type=float, default=24.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    data = fasta_bytes(synth.make_reads("headline2k", a.reads), a.width)
    window = int(a.window_mib * (1 << 20))
    dev = torch.device("cuda", 0)
    buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    out = {"reads": a.reads, "file_bytes": len(data), "window_bytes": window}

    # the walk first, in a context of its own: its buffers never see the whole file
    free0 = free_bytes()
    eng = mtr_amd.Engine(0)
    walks, per_call, ids, lens, peak, twice = [], [], [], [], 0, 0
    for rep in range(a.warmup + a.reps):
        it, total, calls, ids, lens, peak, twice, pos = eng.walk_fasta_device(buf, window), 0.0, [], [], [], 0, 0, 0
        while True:
            t = time.perf_counter()
            f = next(it, None)
            ms = (time.perf_counter() - t) * 1e3
            if f is None:
                break
            total += ms
            calls.append(round(ms, 3))
            more = f.end == "more"
            n = min(window, len(data) - pos)
            peak = max(peak, parser_bytes(n, f, 1 if more else 0))
            twice += pos + n - f.end_pos if more else 0
            pos = f.end_pos
            ids += f.ids
            lens += f.lens.tolist()
        if rep >= a.warmup:
            walks.append(total)
            per_call = calls
    out["walk"] = {"sum_ms": stats(walks), "calls": len(per_call), "per_call_ms_last_rep": per_call, "bytes_parsed_twice": twice,
                   "parser_peak_bytes": peak, "device_free_fell_by": free0 - free_bytes()}
    eng.close()
    del eng

    free0 = free_bytes()
    eng = mtr_amd.Engine(0)
    whole = []
    try:
        for rep in range(a.warmup + a.reps):
            t = time.perf_counter()
            f = eng.upload_fasta_device(buf)
            if rep >= a.warmup:
                whole.append((time.perf_counter() - t) * 1e3)
    except mtr_amd.MtrError as e:                               # the whole file is too large a batch for this GPU: the walk's figures stand alone
        out["whole"] = {"error": str(e)}
        print(json.dumps(out))
        return 1
    out["whole"] = {"ms": stats(whole), "parser_peak_bytes": parser_bytes(len(data), f), "device_free_fell_by": free0 - free_bytes()}
    ok = f.end == "eof" and f.ids == ids and f.lens.tolist() == lens and len(ids) == a.reads
    out["walk_reads_equal_whole_file"] = ok
    out["walk_over_whole"] = round(out["walk"]["sum_ms"]["median"] / out["whole"]["ms"]["median"], 3)
    eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


if __name__ == "__main__":
    sys.exit(main())
