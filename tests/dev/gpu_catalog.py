#!/usr/bin/env python3
"""Development aid: what the catalogue genotype costs against the dense call, on the headline batch (10 000 reads of ~2 kb, synth "headline2k").
Locus i is read i's own repeat: its unit of 100 bases as the motif, the 48 bases before and after the repeat as the flanks; K = 3, q = 12.
  dense_N_ms     mtr_genotype_loci_device on the first N = 16, 64, 256 loci: the yardstick
  catalog_N_ms   mtr_genotype_catalog_device + the copy on the same loci, and alone at 10 000 and 100 000 loci (the reads' own 10 000 loci padded
                 with seeded random ones)
Per catalogue size also, from mtr_test_catalog_stats: the share of the reads' positions that the filter passes, the seed hits, and the
call's host-clock split into the host's index build and upload, the first scan pass (up to the look that ends it), and the rest.
Every call ends in a stream synchronise; the host clock is around it (the catalogue's host-side index build included).  One warm-up repetition,
then --reps timed ones, the calls alternating within a repetition; medians with min and max.  Prints one JSON line; --out FILE writes it too."""
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
    reads, loci = [], []
    for _ in range(a.reads):
        x, unit = synth.make_read(rng, unit_len, copies, flank, flank)
        reads.append(x)
        loci.append((text(x[flank - FLANK:flank]), text(unit), text(x[len(x) - flank:len(x) - flank + FLANK])))
    pad = np.random.RandomState(2027)
    while len(loci) < max(a.big + [0]):
        loci.append((text(pad.randint(0, 4, size=FLANK)), text(pad.randint(0, 4, size=4)), text(pad.randint(0, 4, size=FLANK))))
    eng = mtr_amd.Engine()
    eng.upload(reads)
    torch.cuda.synchronize()

    def timed(call):
        t0 = time.perf_counter()
        got = call()
        return (time.perf_counter() - t0) * 1e3, got

    small = (16, 64, 256)
    ms = {**{f"dense_{m}_ms": [] for m in small}, **{f"catalog_{m}_ms": [] for m in small + tuple(a.big)}}
    found, parts = {}, {m: [] for m in small + tuple(a.big)}

    def note(m, sg):
        counts, split = eng.test_catalog_stats()
        parts[m].append(split)
        found[m] = {"rows": int(sg.read.numel()), "candidates": sg.candidates, "positions": counts[0], "filter_passed": counts[1], "seed_hits": counts[2],
                    "filter_passed_share": round(counts[1] / max(counts[0], 1), 4)}

    for _ in range(a.reps + 1):
        for m in small:
            t, gt = timed(lambda: eng.genotype_loci(loci[:m], K))
            ms[f"dense_{m}_ms"].append(t)
            t, sg = timed(lambda: eng.genotype_catalog(loci[:m], K, Q))
            ms[f"catalog_{m}_ms"].append(t)
            assert all(torch.equal(x, y) for x, y in zip(sg.to_dense(), gt))
            note(m, sg)
            del gt
        for m in a.big:
            t, sg = timed(lambda: eng.genotype_catalog(loci[:m], K, Q))
            ms[f"catalog_{m}_ms"].append(t)
            note(m, sg)
    out = {"reads": len(reads), "bases": int(sum(len(r) for r in reads)), "max_flank_dist": K, "seed_len": Q, "flank_bases": FLANK, "motif_bases": unit_len}
    out.update({k: stats(v[1:]) for k, v in ms.items()})
    out["found"] = {str(k): v for k, v in found.items()}
    out["catalog_split_ms"] = {str(m): {name: stats([p[k] for p in v[1:]]) for k, name in enumerate(("index_build_and_upload", "first_scan_pass", "rest"))}
                               for m, v in parts.items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
