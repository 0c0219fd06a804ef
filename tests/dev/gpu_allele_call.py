#!/usr/bin/env python3
"""Development aid: what the allele calls cost (Engine.call_alleles: the size call, the allocation of the columns, the writing call), on
synthetic genotype rows already on the device:
  one_locus     10 000 reads x 1 locus, every read spanning: two noisy clusters of copies
  many_loci     10 000 reads x 64 loci, 5 % of the rows spanning
  million       1 000 000 reads x 1 locus, every read spanning (--million 0 leaves it out): the rank's S_l^2 compares at the size for which
                DESIGN.md 7i-6 estimates them from lane counts
Per input: call_ms, and host_ms, the yardstick - what a user does without the call: the four columns copied to the host, the supporting rows
picked, np.lexsort by (value, read) per locus (the split is not even made: a lower bound).  Every call ends synchronised; the host clock is
around it.  One warm-up repetition, then --reps timed ones; medians with min and max.  Prints one JSON line; --out FILE writes it too.
Kernel times come from a run of their own: rocprofv3 --kernel-trace --stats -- python tests/dev/gpu_allele_call.py --reps 2"""
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


def stats(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def rows(rng, n, m, share, dev):
    spanning = (rng.rand(n, m) < share).astype(np.uint8)
    copies = np.where(rng.rand(n, m) < 0.4, 35, 20) + rng.randint(-2, 3, size=(n, m))
    window = np.zeros((n, m, 2), np.int32)
    window[:, :, 0] = rng.randint(0, 1000, size=(n, m))
    window[:, :, 1] = window[:, :, 0] + 3 * copies + rng.randint(-1, 2, size=(n, m))
    fields = np.zeros((n, m, 8), np.int32)
    fields[:, :, 3] = copies
    ratio = rng.uniform(0.6, 1.0, size=(n, m)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return mtr_amd.Genotypes(t(spanning), None, None, t(window), t(fields), None, t(ratio))


def host_way(gt, min_ratio):
    sp, w, f, ra = (c.cpu().numpy() for c in (gt.spanning, gt.window, gt.fields, gt.ratio))
    ok = (sp == 1) & ((w[:, :, 1] == w[:, :, 0]) | (ra >= np.float32(min_ratio)))
    total = 0
    for l in range(sp.shape[1]):
        rd = np.nonzero(ok[:, l])[0]
        total += len(np.lexsort((rd, f[rd, l, 3])))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--million", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    eng = mtr_amd.Engine()
    dev = torch.device("cuda", eng.device)
    rng = np.random.RandomState(2026)
    inputs = {"one_locus": rows(rng, 10000, 1, 1.0, dev), "many_loci": rows(rng, 10000, 64, 0.05, dev)}
    if a.million:
        inputs["million"] = rows(rng, 1000000, 1, 1.0, dev)
    torch.cuda.synchronize()
    out = {"min_ratio": 0.7, "rule": [3, 20, 2], "measure": "copies"}
    for name, gt in inputs.items():
        call_ms, host_ms, calls, S = [], [], None, 0
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            calls = eng.call_alleles(gt, "copies", 0.7, 3, 20, 2)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            S = host_way(gt, 0.7)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert int(calls.support_off[-1]) == S
        out[name] = {"reads": int(gt.spanning.shape[0]), "loci": int(gt.spanning.shape[1]), "support": S, "call_ms": stats(call_ms[1:]), "host_ms": stats(host_ms[1:]),
                     "zygosity": np.bincount(calls.zygosity.cpu().numpy(), minlength=3).tolist(), "first_call": calls.call[0].cpu().tolist(),
                     "first_support": calls.call_support[0].cpu().tolist()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
