#!/usr/bin/env python3
"""Development aid: what the flank search and the locus genotyping cost, on the headline batch (10 000 reads of ~2 kb, synth "headline2k").
Calls on the same batch, alternating within a repetition:
  search_u16_ms   mtr_search_motifs_device, one seeded random motif of 16 bases, both strands, scores (1, 1, 1): the yardstick
  flanks_M_ms     mtr_search_flanks_device, one seeded random pattern of M = 20, 32, 33 and 64 bases, both strands
  flanks_32w64_ms the 32-base pattern again with MTR_TEST_FLANK_WORD=64: the same work through the 64-bit scan
  genotype_ms     mtr_genotype_loci_device, K = 3, one locus taken from the first read's own construction: its unit of 100 bases as the motif,
                  the 32 bases before and after its repeat as the flanks
All into preallocated columns.  Every call ends in a stream synchronise; the host clock is around it.  One warm-up repetition, then --reps
timed ones; medians with min and max.  Prints one JSON line; --out FILE writes it too.
Kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_flank_search.py --reps 2"""
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

LENGTHS = (20, 32, 33, 64)


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def text(codes):
    return "".join("ACGT"[int(c)] for c in codes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    unit_len, copies, flank, _, seed = synth.CONFIGS["headline2k"]
    reads = [c for _, c in synth.make_reads("headline2k", a.reads, seed)]
    first, unit = synth.make_read(np.random.RandomState(seed), unit_len, copies, flank, flank)       # the first read again, with its unit
    assert np.array_equal(first, reads[0])
    locus = (text(first[flank - 32:flank]), text(unit), text(first[len(first) - flank:len(first) - flank + 32]))
    n = len(reads)
    eng = mtr_amd.Engine()
    eng.upload(reads)
    dev = torch.device("cuda", eng.device)
    lib, h = eng.lib, eng.h
    rng = np.random.RandomState(2026)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)      # noqa: E731
    u8 = lambda k: torch.empty(k, dtype=torch.uint8, device=dev)       # noqa: E731
    f32 = lambda k: torch.empty(k, dtype=torch.float32, device=dev)    # noqa: E731
    mhits, fhits = (i32(n * 8), i32(n), f32(n), u8(n)), (i32(n), i32(n), i32(n), u8(n))
    gcols = (u8(n), u8(n), i32(2 * n), i32(2 * n), i32(8 * n), i32(n), f32(n))
    torch.cuda.synchronize()
    count = C.c_int64()

    def timed(call):
        t0 = time.perf_counter()
        st = call()
        ms = (time.perf_counter() - t0) * 1e3
        assert st == 0 and count.value == n, (st, lib.mtr_last_error(h))
        return ms

    motif = mtr_amd.pack_ids([text(rng.randint(0, 4, size=16))])
    patterns = {m: mtr_amd.pack_ids([text(rng.randint(0, 4, size=m))]) for m in LENGTHS}
    seqs = mtr_amd.pack_ids(list(locus))

    def search():
        dst = mtr_amd.CMotifHitsDst(*[t.data_ptr() for t in mhits], n)
        return timed(lambda: lib.mtr_search_motifs_device(h, motif[0].ctypes.data, motif[1].ctypes.data, 1, 1, 1, 1, 1, C.byref(dst), C.byref(count)))

    def flanks(m, word=None):
        dst = mtr_amd.CFlankHitsDst(*[t.data_ptr() for t in fhits], n)
        if word:
            os.environ["MTR_TEST_FLANK_WORD"] = word
        try:
            return timed(lambda: lib.mtr_search_flanks_device(h, patterns[m][0].ctypes.data, patterns[m][1].ctypes.data, 1, 1, C.byref(dst), C.byref(count)))
        finally:
            os.environ.pop("MTR_TEST_FLANK_WORD", None)

    def genotype():
        dst = mtr_amd.CGenotypesDst(*[t.data_ptr() for t in gcols], n)
        return timed(lambda: lib.mtr_genotype_loci_device(h, seqs[0].ctypes.data, seqs[1].ctypes.data, 1, 3, 1, 1, 1, C.byref(dst), C.byref(count)))

    ms = {"search_u16_ms": [], **{f"flanks_{m}_ms": [] for m in LENGTHS}, "flanks_32w64_ms": [], "genotype_ms": []}
    for _ in range(a.reps + 1):
        ms["search_u16_ms"].append(search())
        for m in LENGTHS:
            ms[f"flanks_{m}_ms"].append(flanks(m))
        ms["flanks_32w64_ms"].append(flanks(32, "64"))
        ms["genotype_ms"].append(genotype())
    out = {"reads": n, "bases": int(sum(len(r) for r in reads)), "both_strands": True, "max_flank_dist": 3,
           "locus": {"left": locus[0], "motif_bases": len(locus[1]), "right": locus[2]}}
    out.update({k: stats(v[1:]) for k, v in ms.items()})
    sp = gcols[0].cpu().numpy()
    out["spanning_reads"] = int(sp.sum())
    out["first_read"] = {"spanning": int(sp[0]), "window": gcols[3][:2].cpu().tolist(), "copies": int(gcols[4][3]), "flank_dist": gcols[2][:2].cpu().tolist()}
    out["flanks_32_over_search_u16"] = round(out["flanks_32_ms"]["median"] / out["search_u16_ms"]["median"], 3)
    out["word64_over_word32"] = round(out["flanks_32w64_ms"]["median"] / out["flanks_32_ms"]["median"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
