#!/usr/bin/env python3
"""Development aid: what the partial genotype at catalogue scale costs against the dense call.  Two measurements:
  (a) cut reads   the headline batch (10 000 reads of ~2 kb, synth "headline2k") with every read cut inside its repeat - the even reads to the
                  prefix that keeps the left flank and half the repeat, the odd reads to the suffix that keeps the right flank and half the
                  repeat.  Locus i is read i's own repeat: the 48 bases before and after it as the flanks, the first 32 bases of its 100-base
                  unit as the motif (the call takes motifs of at most 32 bases); K = 3, q = 12.
                    dense_N_ms     mtr_genotype_partial_device of the library under test on the first N = 16, 64, 256 loci: the yardstick (beyond that its reads x loci
                                   buffers do not fit: it cannot run)
                    sparse_N_ms    mtr_genotype_partial_catalog_device + the copy on the same loci, and alone at 10 000 and 100 000 loci (the
                                   reads' own 10 000 loci padded with seeded random ones)
  (b) all tasks   tests/dev/gpu_partial.py's batch (b): every read a task of one locus, a shared 20-base flank, then a 16-base motif to the
                  read's end with 8 % substitutions; K = 0, q = 16.  The price of the per-lane motif:
                    dense_all_ms   mtr_genotype_partial_device (mtr_k_ext_lanes<16>: the motif in scalar registers)
                    sparse_all_ms  mtr_genotype_partial_catalog_device + the copy (mtr_k_ptc_ext<16>: the motif per lane)
Per sparse call also, from mtr_test_partial_catalog_stats: the seed positions, those the filter passed, the seed hits, and the call's host-clock
split into the host's index build and upload, the first scan pass (up to the look that ends it), and the rest.
Every call ends in a stream synchronise; the host clock is around it (the sparse call's host-side index build included).  One warm-up
repetition, then --reps timed ones, the calls alternating within a repetition; medians with min and max.  Prints one JSON line; --out FILE
writes it too."""
import argparse
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

K, Q, FLANK = 3, 12, 48


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def text(codes):
    return "".join("ACGT"[int(c)] for c in codes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, nargs="*", default=[10000, 100000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    unit_len, copies, flank, _, seed = synth.CONFIGS["headline2k"]
    rng = np.random.RandomState(seed)
    whole, cut, loci = [], [], []
    for i in range(a.reads):
        x, unit = synth.make_read(rng, unit_len, copies, flank, flank)
        whole.append(x)
        half = (len(x) - 2 * flank) // 2
        cut.append(x[:flank + half] if i % 2 == 0 else x[len(x) - flank - half:])
        loci.append((text(x[flank - FLANK:flank]), text(unit[:32]), text(x[len(x) - flank:len(x) - flank + FLANK])))
    pad = np.random.RandomState(2027)
    while len(loci) < max(a.big + [0]):
        loci.append((text(pad.randint(0, 4, size=FLANK)), text(pad.randint(0, 4, size=4)), text(pad.randint(0, 4, size=FLANK))))
    rng = np.random.RandomState(2027)
    shared, motif = rng.randint(0, 4, size=20).astype(np.uint8), rng.randint(0, 4, size=16).astype(np.uint8)
    tasks = []
    for r in whole:
        rep = np.tile(motif, len(r) // 16 + 1)[:len(r) - 20].copy()
        hit = rng.rand(len(rep)) < 0.08
        rep[hit] = (rep[hit] + 1 + rng.randint(0, 3, size=int(hit.sum()))) & 3
        tasks.append(np.concatenate([shared, rep]).astype(np.uint8))
    one = [(text(shared), text(motif), text(rng.randint(0, 4, size=20)))]

    eng_a, eng_b = mtr_amd.Engine(), mtr_amd.Engine()
    eng_a.upload(cut)
    eng_b.upload(tasks)
    torch.cuda.synchronize()

    def timed(call):
        t0 = time.perf_counter()
        got = call()
        return (time.perf_counter() - t0) * 1e3, got

    small = (16, 64, 256)
    ms = {**{f"dense_{m}_ms": [] for m in small}, **{f"sparse_{m}_ms": [] for m in small + tuple(a.big)}, "dense_all_ms": [], "sparse_all_ms": []}
    found, parts = {}, {m: [] for m in small + tuple(a.big) + ("all",)}

    def note(eng, m, spg, **more):
        counts, split = eng.test_partial_catalog_stats()
        parts[m].append(split)
        found[m] = {"rows": int(spg.read.numel()), "candidates": spg.candidates, "open_rows": int(spg.open.sum()), "positions": counts[0], "filter_passed": counts[1],
                    "seed_hits": counts[2], **more}

    for _ in range(a.reps + 1):
        for m in small:
            t, pg = timed(lambda: eng_a.genotype_partial(loci[:m], K))
            ms[f"dense_{m}_ms"].append(t)
            t, spg = timed(lambda: eng_a.genotype_partial_catalog(loci[:m], K, Q))
            ms[f"sparse_{m}_ms"].append(t)
            note(eng_a, m, spg)
            assert all(torch.equal(x, y) for x, y in zip(spg.to_dense(), pg))
            del pg
        for m in a.big:
            t, spg = timed(lambda: eng_a.genotype_partial_catalog(loci[:m], K, Q))
            ms[f"sparse_{m}_ms"].append(t)
            note(eng_a, m, spg)
        t, pg = timed(lambda: eng_b.genotype_partial(one, 0))
        ms["dense_all_ms"].append(t)
        t, spg = timed(lambda: eng_b.genotype_partial_catalog(one, 0, 16))
        ms["sparse_all_ms"].append(t)
        note(eng_b, "all", spg, window_bases=int((spg.window[:, 1] - spg.window[:, 0]).sum()), copies_median=float(spg.ext[:, 2].float().median()))
        assert all(torch.equal(x, y) for x, y in zip(spg.to_dense(), pg))
    out = {"reads": len(cut), "cut_bases": int(sum(len(r) for r in cut)), "task_bases": int(sum(len(r) for r in tasks)), "max_flank_dist": K, "seed_len": Q,
           "flank_bases": FLANK, "motif_bases": 32, "scores": [1, 1, 1], "max_tail": 10}
    out.update({k: stats(v[1:]) for k, v in ms.items()})
    out["found"] = {str(k): v for k, v in found.items()}
    out["sparse_all_over_dense_all"] = round(out["sparse_all_ms"]["median"] / out["dense_all_ms"]["median"], 3)
    out["sparse_split_ms"] = {str(m): {name: stats([p[k] for p in v[1:]]) for k, name in enumerate(("index_build_and_upload", "first_scan_pass", "rest"))}
                              for m, v in parts.items()}
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
