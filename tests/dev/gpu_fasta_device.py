#!/usr/bin/env python3
"""Development aid: what parsing FASTA on the device costs on the headline shape (10 000 reads of ~2 kb, synth "headline2k"), once
written as single-line records and once wrapped at 60 columns.  For each file it times
  upload_fasta_device   the file's bytes in a GPU tensor -> the resident batch (mtr_upload_fasta_device + mtr_fasta_index);
  parse_fasta_device    the same bytes -> the reads as text and their index (mtr_parse_fasta_device, sizes call + writing call);
  host_parse_upload     the path without the device parser, for the same bytes: mtrh_parse_chunk_packed on ONE host core over the
                        memory-mapped file, then mtr_upload_batch_packed of its image
by the host clock around the calls (each returns after the device work), then runs the batch after a device and after a host upload
and checks that both give the same wire bytes.  Prints one JSON line; --out FILE writes it there as well.
Kernel time: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_fasta_device.py"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the first Engine: one HIP runtime serves both)
import numpy as np  # noqa: E402

import mtr_amd  # noqa: E402
from mtr_amd import synth  # noqa: E402
from tests import host_util as hu  # noqa: E402
from tests.test_host_driver import Batch, File  # noqa: E402  (ctypes mirrors of mtrh_batch / mtrh_file)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def fasta_bytes(named, width):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts = []
    for rid, codes in named:
        s = acgt[codes].tobytes()
        body = s if not width else b"\n".join(s[i:i + width] for i in range(0, len(s), width))
        parts.append(b">" + str(rid).encode() + b"\n" + body + b"\n")
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    hu.build_host()
    host = C.CDLL(os.path.join(hu.HOST, "libmtr_host.so"))
    host.mtrh_file_open.argtypes = [C.POINTER(File), C.c_char_p]
    host.mtrh_file_close.argtypes = [C.POINTER(File)]
    host.mtrh_parse_chunk_packed.restype = C.POINTER(Batch)
    host.mtrh_parse_chunk_packed.argtypes = [C.POINTER(File), C.c_size_t, C.c_size_t, C.c_int, C.c_int64]
    host.mtrh_batch_free.argtypes = [C.POINTER(Batch)]

    named = synth.make_reads("headline2k", a.reads)
    dev = torch.device("cuda", 0)
    eng = mtr_amd.Engine(0)
    out = {"reads": len(named), "bases": int(sum(len(c) for _, c in named))}
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        for label, width in (("single_line", 0), ("wrapped_60", 60)):
            data = fasta_bytes(named, width)
            path = os.path.join(tmp, label + ".fa")
            with open(path, "wb") as fh:
                fh.write(data)
            buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
            torch.cuda.synchronize()
            f = File()
            assert host.mtrh_file_open(C.byref(f), path.encode()) == 0

            def host_parse_upload():
                head = host.mtrh_parse_chunk_packed(C.byref(f), 0, len(data), 1 << 30, 1 << 40)
                b = head.contents
                assert b.n == len(named) and not b.next
                eng._check(eng.lib.mtr_upload_batch_packed(eng.h, b.packed, b.n_words, b.woff, b.lens, b.n), "mtr_upload_batch_packed")
                eng.n_reads = b.n
                host.mtrh_batch_free(head)

            res = {"file_bytes": len(data),
                   "upload_fasta_device_ms": timed(lambda: eng.upload_fasta_device(buf), a.warmup, a.reps),
                   "parse_fasta_device_ms": timed(lambda: eng.parse_fasta_device(buf), a.warmup, a.reps),
                   "host_parse_upload_ms": timed(host_parse_upload, a.warmup, a.reps)}
            fa = eng.upload_fasta_device(buf)
            eng.run()
            got = eng.fetch_packed()[0]
            host_parse_upload()
            eng.run()
            res["identical_wire_bytes"] = got == eng.fetch_packed()[0] and fa.end == "eof" and len(fa.ids) == len(named)
            ok = ok and res["identical_wire_bytes"]
            host.mtrh_file_close(C.byref(f))
            out[label] = res
    eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
