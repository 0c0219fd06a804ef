"""Probe: the call time of Engine.genotype_quality at catalogue scale, several alignments per wavefront against one.

    python tests/dev/gpu_genotype_quality.py [--loci 10000] [--members 30] [--bases 60] [--band-extra 16] [--out profiles/genotype_quality_probe.json]

The workload is tests/dev/gpu_seq_calls.py's: --loci loci of --members supporting reads each, two alleles of one length ten substitutions apart,
every read's window its allele with two substitutions and up to three bases cut off its end (lengths --bases - 3 .. --bases), qualities 2 .. 40;
the reads alternate between the alleles and are scored against both true sequences.  The whole call is the host clock around a synchronised
call: one warm-up, the median of five with min and max, with MTR_TEST_GQ_ROWS unset and "0", alternating in one process; both must return
the same columns.  The kernels' own times come from a run of this script under a kernel trace, which slows the host and is a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -- python tests/dev/gpu_genotype_quality.py --rounds 2 --modes several      (and again with --modes one)

(mtr_k_gq_score<4, 1> = four per wavefront, <2, 1> = two, <1, 1> = one with one pair of diagonals per lane - with the switch at 0 the first two
buckets' tasks too - <1, 2> = one with two pairs, mtr_k_gq_tasks, mtr_k_gq_locus).  The band is |m - n| + 2 * band_extra + 1 diagonals: the
default band_extra 16 gives 33 .. 36, two tasks per wavefront; --band-extra 14 gives 29 .. 32, four."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import mtr_amd  # noqa: E402
from gpu_seq_calls import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--members", type=int, default=30)
    ap.add_argument("--bases", type=int, default=60)
    ap.add_argument("--band-extra", type=int, nargs="+", default=[16, 14])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--modes", default="several,one", help="several = four or two alignments per wavefront, one = MTR_TEST_GQ_ROWS=0; under a kernel trace give one of them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genotype_quality_probe.json"))
    args = ap.parse_args()
    case, lens = workload(args.loci, args.members, args.bases)
    rng = np.random.default_rng(2)
    # the alleles' sequences: workload()'s truth, drawn again with its seed (allele 1 = allele 0 with ten substitutions)
    r2 = np.random.default_rng(1)
    truth = r2.integers(0, 4, size=(args.loci, 2, args.bases)).astype(np.uint8)
    at = np.argsort(r2.random((args.loci, args.bases)), axis=1)[:, :10]
    truth[:, 1] = truth[:, 0]
    for k in range(10):
        truth[np.arange(args.loci), 1, at[:, k]] = (truth[np.arange(args.loci), 0, at[:, k]] + 1 + k % 3) % 4
    S = args.loci * args.members
    eng = mtr_amd.Engine()
    dev = torch.device("cuda", eng.device)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    sg = SimpleNamespace(n_loci=args.loci, read=put(case["read"]), locus=put(case["locus"]))
    win = mtr_amd.GenotypeWindows(put(case["win_off"]), put(case["win_bases"]))
    qual = put(rng.integers(2, 41, size=len(case["win_bases"])).astype(np.uint8))
    # the support lists as the consensus wants them: allele 0's reads (the even ones) in front
    order = np.concatenate([np.arange(0, args.members, 2), np.arange(1, args.members, 2)]).astype(np.int32)
    calls = SimpleNamespace(support_off=put(case["support_off"]), read=put(np.tile(order, args.loci)),
                            allele=put(np.tile((order % 2).astype(np.uint8), args.loci)), zygosity=put(np.full(args.loci, 2, np.uint8)))
    cons = SimpleNamespace(off=put(np.arange(2 * args.loci + 1, dtype=np.int64) * args.bases), bases=put(truth.reshape(-1)))
    modes = args.modes.split(",")
    rows = []
    for extra in args.band_extra:
        width = np.abs(args.bases - lens) + 2 * extra + 1
        buckets = [int(2 * ((width > lo) & (width <= hi)).sum()) for lo, hi in ((0, 32), (32, 64), (64, 128), (128, 256))]
        times, outs = {mode: [] for mode in modes}, {}
        for _ in range(args.rounds):
            for mode in modes:
                if mode == "one":
                    os.environ["MTR_TEST_GQ_ROWS"] = "0"
                else:
                    os.environ.pop("MTR_TEST_GQ_ROWS", None)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                outs[mode] = eng.genotype_quality(sg, win, qual, calls, cons, band_extra=extra)
                torch.cuda.synchronize(dev)
                times[mode].append((time.perf_counter() - t0) * 1e3)
        first, last = outs[modes[0]], outs[modes[-1]]
        same = all(torch.equal(x, y) for x, y in zip(first, last))
        gt = first.gt.cpu().numpy()
        true_side = bool((first.best.cpu().numpy() == np.tile(order % 2, args.loci)).all())
        row = dict(loci=args.loci, members=args.members, bases=args.bases, band_extra=extra, tasks=2 * S, tasks_by_bucket=buckets, same_columns=same,
                   gt_counts=[int((gt == g).sum()) for g in (0, 1, 2)], every_best_is_the_true_side=true_side, gq_median=float(np.median(first.gq.cpu().numpy())))
        for mode in times:
            ms = times[mode][1:] or times[mode]
            row.update({f"{mode}_ms_median": statistics.median(ms), f"{mode}_ms_min": min(ms), f"{mode}_ms_max": max(ms)})
        print(json.dumps(row), flush=True)
        rows.append(row)
        assert same
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="Engine.genotype_quality whole, several alignments per wavefront against one (MTR_TEST_GQ_ROWS=0)", rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
