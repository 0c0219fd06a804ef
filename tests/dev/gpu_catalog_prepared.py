#!/usr/bin/env python3
"""Development aid: what a prepared catalogue saves per batch, on the headline batch (10 000 reads of ~2 kb, synth "headline2k"), with
tests/dev/gpu_catalog.py's loci (locus i is read i's own repeat, padded with seeded random loci), K = 3, q = 12, at 256, 10 000 and 100 000 loci.
  build_N_ms            Engine.build_catalog by the host clock (the Python packing of the strings included), and build_split_ms: the C call's own
                        clock over the host's pass over the lengths, the uploads, the device build (mtr_test_catalog_build_stats)
  text_index_N_ms       the index time mtr_test_catalog_stats reports for the text-taking call on the same loci: the host build it replaces
  text_N_ms / prepared_N_ms, text_partial_N_ms / prepared_partial_N_ms
                        genotype_catalog against genotype_prepared, genotype_partial_catalog against genotype_partial_prepared: each call with
                        its copy, ended by a stream synchronise, the host clock around it; the four alternate within a repetition
  prepared_again_N_ms   genotype_prepared once more, straight after: a text-taking call in between makes the context derive and upload the lane
                        slots again (one upload per catalogue and lane_max otherwise); this is the call of a run over batches
  *_rest_ms             the text-taking and the prepared genotype's "rest of the call" (mtr_test_catalog_stats' third clock)
Run it once with MTR_LIB naming the parent's build of the library: that build has no prepared catalogue, and the script then measures the
text-taking calls alone, which is what "the text-taking calls have not slowed" is read from.  One warm-up repetition, then --reps timed ones;
medians with min and max.  Prints one JSON line; --out FILE writes it too."""
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 10000, 100000])
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
    while len(loci) < max(a.sizes + [0]):
        loci.append((text(pad.randint(0, 4, size=FLANK)), text(pad.randint(0, 4, size=4)), text(pad.randint(0, 4, size=FLANK))))
    eng = mtr_amd.Engine()
    eng.upload(reads)
    torch.cuda.synchronize()
    prepared = hasattr(eng.lib, "mtr_catalog_create")
    # the partial calls take motifs of at most 32 bases: the reads' own 100-base units give way to their first 32 bases there
    partial_loci = [(a_, m[:32], b_) for a_, m, b_ in loci]

    def timed(call):
        t0 = time.perf_counter()
        got = call()
        return (time.perf_counter() - t0) * 1e3, got

    ms, split, info = {}, {}, {}
    add = lambda key, v: ms.setdefault(key, []).append(v)      # noqa: E731
    for rep in range(a.reps + 1):
        for m in a.sizes:
            sub, psub = loci[:m], partial_loci[:m]
            if prepared:
                t, cat = timed(lambda: eng.build_catalog(sub, K, Q))
                add(f"build_{m}_ms", t)
                split.setdefault(m, []).append(eng.test_catalog_build_stats())
                pcat = eng.build_catalog(psub, K, Q)
                info[m] = cat.info._asdict()
            t, sg = timed(lambda: eng.genotype_catalog(sub, K, Q))
            add(f"text_{m}_ms", t)
            index_ms, _, rest_ms = eng.test_catalog_stats()[1]
            add(f"text_index_{m}_ms", index_ms)
            add(f"text_rest_{m}_ms", rest_ms)
            if prepared:
                t, got = timed(lambda: eng.genotype_prepared(cat))
                add(f"prepared_{m}_ms", t)
                add(f"prepared_rest_{m}_ms", eng.test_catalog_stats()[1][2])
                assert all(torch.equal(x, y) for x, y in zip(got[2:11], sg[2:11])) and got.candidates == sg.candidates
                t, got = timed(lambda: eng.genotype_prepared(cat))      # the call of a run: no text-taking call since the last one, the lane slots are in the context
                add(f"prepared_again_{m}_ms", t)
                add(f"prepared_again_rest_{m}_ms", eng.test_catalog_stats()[1][2])
                assert all(torch.equal(x, y) for x, y in zip(got[2:11], sg[2:11]))
            t, spg = timed(lambda: eng.genotype_partial_catalog(psub, K, Q))
            add(f"text_partial_{m}_ms", t)
            add(f"text_partial_index_{m}_ms", eng.test_partial_catalog_stats()[1][0])
            if prepared:
                t, got = timed(lambda: eng.genotype_partial_prepared(pcat))
                add(f"prepared_partial_{m}_ms", t)
                assert all(torch.equal(x, y) for x, y in zip(got[2:11], spg[2:11])) and got.candidates == spg.candidates
                cat.close(), pcat.close()
    out = {"library": os.path.basename(mtr_amd.LIB_PATH), "has_prepared_catalogue": prepared, "reads": len(reads), "bases": int(sum(len(r) for r in reads)),
           "max_flank_dist": K, "seed_len": Q, "flank_bases": FLANK}
    out.update({k: stats(v[1:]) for k, v in ms.items()})
    out["build_split_ms"] = {str(m): {name: stats([p[k] for p in v[1:]]) for k, name in enumerate(("host_pass", "uploads", "device_build"))} for m, v in split.items()}
    out["catalogue"] = {str(m): v for m, v in info.items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
