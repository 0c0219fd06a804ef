#!/usr/bin/env python3
"""Development aid: what the known-motif search costs on the headline batch (10 000 reads of ~2 kb, synth "headline2k"), and whether its lane
path (one DP per lane, mtr_k_motif_lanes) beats its wave path (one DP per wavefront through dp_wrap, mtr_k_motif_waves) on short motifs.
Per motif length U - one seeded random motif, both strands, scores (1, 1, 1) - three ways to the same alignments, alternating within a
repetition:
  lane_ms       mtr_search_motifs_device with MTR_TEST_MOTIF_LANE_MAX=32: the lane path takes every U up to the largest bucket
  wave_ms       the same call with MTR_TEST_MOTIF_LANE_MAX=0
  test_dp_ms    mtr_test_wrap_dp on host task lists, the only route to "align this unit to that read" before this entry point: the forward motif
                and its reverse complement against rows 1 .. L - 1 of every read (its window cannot name a read's first base), results to the host
The search calls write into preallocated columns and end in a stream synchronise; the host clock is around the call.  One warm-up repetition,
then --reps timed ones; medians with min and max.  The lane and wave columns are compared once (they must be equal).  Prints one JSON line;
--out FILE writes it too.
Kernel times: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_motif_search.py --reps 2"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lengths", default="2,3,6,8,16,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    reads = [c for _, c in synth.make_reads("headline2k", a.reads, synth.CONFIGS["headline2k"][4])]
    n = len(reads)
    eng = mtr_amd.Engine()
    eng.upload(reads)
    dev = torch.device("cuda", eng.device)
    lib, h = eng.lib, eng.h
    rng = np.random.RandomState(2026)
    out = {"reads": n, "bases": int(sum(len(r) for r in reads)), "scores": [1, 1, 1], "both_strands": True, "rows": []}
    for U in [int(v) for v in a.lengths.split(",")]:
        codes = rng.randint(0, 4, size=U).astype(np.uint8)
        motif = "".join("ACGT"[c] for c in codes)
        data, off = mtr_amd.pack_ids([motif])
        cols = {k: (torch.empty(n * 8, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                    torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)) for k in ("lane", "wave")}
        torch.cuda.synchronize()
        nh = C.c_int64()

        def search(which):
            os.environ["MTR_TEST_MOTIF_LANE_MAX"] = "32" if which == "lane" else "0"
            dst = mtr_amd.CMotifHitsDst(*[t.data_ptr() for t in cols[which]], n)
            t0 = time.perf_counter()
            st = lib.mtr_search_motifs_device(h, data.ctypes.data, off.ctypes.data, 1, 1, 1, 1, 1, C.byref(dst), C.byref(nh))
            ms = (time.perf_counter() - t0) * 1e3
            assert st == 0 and nh.value == n, (st, lib.mtr_last_error(h))
            return ms

        tasks = [(i, 0, len(r) - 2, u, 1, 1, 1) for u in (codes, (3 - codes)[::-1].copy()) for i, r in enumerate(reads)]

        def test_dp():
            t0 = time.perf_counter()
            eng.test_wrap_dp(tasks)
            return (time.perf_counter() - t0) * 1e3

        ms = {"lane_ms": [], "wave_ms": [], "test_dp_ms": []}
        for _ in range(a.reps + 1):
            ms["lane_ms"].append(search("lane"))
            ms["wave_ms"].append(search("wave"))
            ms["test_dp_ms"].append(test_dp())
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(cols["lane"], cols["wave"]))
        row = {"U": U, "motif": motif, "hits_with_score": int((cols["lane"][1] > 0).sum()), "lane_equals_wave": bool(same)}
        row.update({k: stats(v[1:]) for k, v in ms.items()})
        row["lane_faster"] = row["lane_ms"]["median"] < row["wave_ms"]["median"]
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    os.environ.pop("MTR_TEST_MOTIF_LANE_MAX", None)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
