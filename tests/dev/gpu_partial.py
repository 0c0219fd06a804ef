#!/usr/bin/env python3
"""Development aid: what the partial genotype costs, on the headline batch (10 000 reads of ~2 kb, synth "headline2k").  Two measurements:
  (a) few tasks   mtr_genotype_partial_device, K = 3, on the headline batch itself, one locus taken from the first read's own construction: the 32
                  bases before and after its repeat as the flanks, the first 32 bases of its 100-base unit as the motif (the call takes motifs
                  of at most 32 bases).  Hardly a read holds a flank: the call is its flank step.
                    partial_headline_ms
  (b) all tasks   a batch of the headline's read lengths in which every read is a task whose window is nearly the whole read: a shared 20-base
                  flank, then a 16-base motif repeated to the read's end with 8 % of the bases substituted.  Alternating within a repetition:
                    partial_all_ms      mtr_genotype_partial_device, K = 0, scores (1, 1, 1)
                    search_u16_ms       mtr_search_motifs_device with that motif, ONE strand, scores (1, 1, 1): the yardstick - the same rows and
                                        columns, with a byte per cell stored and a traceback walked
All into preallocated columns.  Every call ends in a stream synchronise; the host clock is around it.  One warm-up repetition, then --reps
timed ones; medians with min and max.  Prints one JSON line; --out FILE writes it too.
Kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_partial.py --reps 2"""
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
    locus = (text(first[flank - 32:flank]), text(unit[:32]), text(first[len(first) - flank:len(first) - flank + 32]))
    n = len(reads)
    rng = np.random.RandomState(2027)
    shared, motif = rng.randint(0, 4, size=20).astype(np.uint8), rng.randint(0, 4, size=16).astype(np.uint8)
    tasks = []
    for r in reads:
        rep = np.tile(motif, len(r) // 16 + 1)[:len(r) - 20].copy()
        hit = rng.rand(len(rep)) < 0.08
        rep[hit] = (rep[hit] + 1 + rng.randint(0, 3, size=int(hit.sum()))) & 3
        tasks.append(np.concatenate([shared, rep]).astype(np.uint8))
    other = text(rng.randint(0, 4, size=20))

    eng_a, eng_b = mtr_amd.Engine(), mtr_amd.Engine()
    eng_a.upload(reads)
    eng_b.upload(tasks)
    dev = torch.device("cuda", eng_a.device)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)      # noqa: E731
    u8 = lambda k: torch.empty(k, dtype=torch.uint8, device=dev)       # noqa: E731
    f32 = lambda k: torch.empty(k, dtype=torch.float32, device=dev)    # noqa: E731
    mhits = (i32(n * 8), i32(n), f32(n), u8(n))
    pcols = {k: (u8(n), u8(n), i32(n), i32(2 * n), i32(6 * n), f32(n), u8(n)) for k in "ab"}
    torch.cuda.synchronize()
    count = C.c_int64()

    def timed(eng, call):
        t0 = time.perf_counter()
        st = call()
        ms = (time.perf_counter() - t0) * 1e3
        assert st == 0 and count.value == n, (st, eng.lib.mtr_last_error(eng.h))
        return ms

    seqs_a, seqs_b, mot = mtr_amd.pack_ids(list(locus)), mtr_amd.pack_ids([text(shared), text(motif), other]), mtr_amd.pack_ids([text(motif)])

    def partial(eng, key, seqs, K):
        dst = mtr_amd.CPartialDst(*[t.data_ptr() for t in pcols[key]], n)
        return timed(eng, lambda: eng.lib.mtr_genotype_partial_device(eng.h, seqs[0].ctypes.data, seqs[1].ctypes.data, 1, K, 1, 1, 1, 10, C.byref(dst), C.byref(count)))

    def search():
        dst = mtr_amd.CMotifHitsDst(*[t.data_ptr() for t in mhits], n)
        return timed(eng_b, lambda: eng_b.lib.mtr_search_motifs_device(eng_b.h, mot[0].ctypes.data, mot[1].ctypes.data, 1, 1, 1, 1, 0, C.byref(dst), C.byref(count)))

    ms = {"partial_headline_ms": [], "partial_all_ms": [], "search_u16_ms": []}
    for _ in range(a.reps + 1):
        ms["partial_headline_ms"].append(partial(eng_a, "a", seqs_a, 3))
        ms["partial_all_ms"].append(partial(eng_b, "b", seqs_b, 0))
        ms["search_u16_ms"].append(search())
    out = {"reads": n, "bases": int(sum(len(r) for r in reads)), "task_bases": int(sum(len(r) for r in tasks)), "scores": [1, 1, 1], "max_tail": 10,
           "locus": {"left": locus[0], "motif": locus[1], "right": locus[2], "max_flank_dist": 3}}
    out.update({k: stats(v[1:]) for k, v in ms.items()})
    pa, pb = [[t.cpu().numpy() for t in pcols[k]] for k in "ab"]
    eb = pb[4].reshape(n, 6)
    out["headline_partial_rows"] = int(pa[0].sum())
    out["all_partial_rows"], out["all_open_rows"] = int(pb[0].sum()), int(pb[6].sum())
    out["all_window_bases"] = int((pb[3].reshape(n, 2)[:, 1] - pb[3].reshape(n, 2)[:, 0]).sum())
    out["all_copies_median"], out["all_ratio_median"] = float(np.median(eb[:, 2])), round(float(np.median(pb[5])), 4)
    out["search_copies_median"] = float(np.median(mhits[0].cpu().numpy().reshape(n, 8)[:, 3]))
    out["partial_all_over_search_u16"] = round(out["partial_all_ms"]["median"] / out["search_u16_ms"]["median"], 3)
    out["kernel_trace"] = "none taken"
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng_a.close()
    eng_b.close()


if __name__ == "__main__":
    main()
