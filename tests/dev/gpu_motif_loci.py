#!/usr/bin/env python3
"""Development aid: what the known-motif locus search costs next to the known-motif search, on the headline batch (10 000 reads of ~2 kb, synth
"headline2k").  Per motif length U - one seeded random motif, both strands, scores (1, 1, 1) - three calls on the same batch, alternating within a
repetition:
  search_ms     mtr_search_motifs_device into preallocated columns
  loci_r1_ms    mtr_search_motif_loci_device with max_rounds = 1, then mtr_motif_loci_copy_device into preallocated columns
  loci_r16_ms   the same with max_rounds = 16
min_score is the median of the search's scores over the reads, so that about one locus per read passes; the row says which it was, how many
loci each call found and how many pairs max_rounds left open.  Every call ends in a stream synchronise; the host clock is around it.  One warm-up
repetition, then --reps timed ones; medians with min and max.  Prints one JSON line; --out FILE writes it too.
Kernel times: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_motif_loci.py --reps 2"""
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
    ap.add_argument("--lengths", default="2,3,6,16")
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
        motif = "".join("ACGT"[c] for c in rng.randint(0, 4, size=U))
        data, off = mtr_amd.pack_ids([motif])
        hits = (torch.empty(n * 8, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        nh, npairs, nloci = C.c_int64(), C.c_int64(), C.c_int64()

        def search():
            dst = mtr_amd.CMotifHitsDst(*[t.data_ptr() for t in hits], n)
            t0 = time.perf_counter()
            st = lib.mtr_search_motifs_device(h, data.ctypes.data, off.ctypes.data, 1, 1, 1, 1, 1, C.byref(dst), C.byref(nh))
            ms = (time.perf_counter() - t0) * 1e3
            assert st == 0 and nh.value == n, (st, lib.mtr_last_error(h))
            return ms

        search()
        S = max(1, int(hits[1].to(torch.float32).median().item()))
        cap = 64 * n                                                  # room for the copy: the search itself keeps whatever it finds
        cols = (torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(cap * 8, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        found = {}

        def loci(R):
            dst = mtr_amd.CMotifLociDst(*[t.data_ptr() for t in cols], n, cap)
            t0 = time.perf_counter()
            st = lib.mtr_search_motif_loci_device(h, data.ctypes.data, off.ctypes.data, 1, 1, 1, 1, 1, S, R, C.byref(npairs), C.byref(nloci))
            st2 = lib.mtr_motif_loci_copy_device(h, C.byref(dst)) if st == 0 else -1
            ms = (time.perf_counter() - t0) * 1e3
            assert st == 0 and st2 == 0 and npairs.value == n, (st, st2, lib.mtr_last_error(h))
            found[R] = (int(nloci.value), int(cols[5].sum()))
            return ms

        ms = {"search_ms": [], "loci_r1_ms": [], "loci_r16_ms": []}
        for _ in range(a.reps + 1):
            ms["search_ms"].append(search())
            ms["loci_r1_ms"].append(loci(1))
            ms["loci_r16_ms"].append(loci(16))
        row = {"U": U, "motif": motif, "min_score": S, "loci_r1": found[1][0], "open_r1": found[1][1], "loci_r16": found[16][0], "open_r16": found[16][1]}
        row.update({k: stats(v[1:]) for k, v in ms.items()})
        row["r1_over_search"] = round(row["loci_r1_ms"]["median"] / row["search_ms"]["median"], 3)
        row["r16_over_search"] = round(row["loci_r16_ms"]["median"] / row["search_ms"]["median"], 3)
        out["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
