"""Probe: the call time of Engine.call_alleles_by_sequence at catalogue scale, four alignments per wavefront against one.

    python tests/dev/gpu_seq_calls.py [--loci 10000] [--members 30] [--bases 60] [--max-dist 32] [--out profiles/seq_calls_probe.json]

The workload: --loci loci of --members supporting reads each, two alleles of one length ten substitutions apart, every read's window its
allele with two substitutions and up to three bases cut off its end (lengths --bases - 3 .. --bases).  The whole call is the host clock around
a synchronised call: one warm-up, the median of five with min and max, with MTR_TEST_SEQ_ROWS unset and "0", alternating; both must return the
same columns.  The kernels' own times come from a run of this script under a kernel trace, which slows the host and is a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -- python tests/dev/gpu_seq_calls.py --rounds 2 --modes four      (and again with --modes one)

(mtr_k_seq_dist<4, 1> = four per wavefront, <2, 1> = two, <1, 1> = one with one pair of diagonals per lane - with the switch at 0 the first two
buckets' tasks too - <1, 2> = one with two pairs, mtr_k_seq_split).  The script also prints how the pairs fall into the band buckets: with K even
a pair of equal parity of lengths has a band of K + 1 diagonals, so at K = 32 only the pairs whose lengths differ by an odd number fit a row of
16 lanes; the others run two per wavefront."""
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

import torch  # noqa: E402

import mtr_amd  # noqa: E402


def workload(n_loci, members, bases, seed=1):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, 4, size=(n_loci, 2, bases)).astype(np.uint8)
    at = np.argsort(rng.random((n_loci, bases)), axis=1)[:, :10]                  # allele 1 = allele 0 with ten substitutions
    truth[:, 1] = truth[:, 0]
    for k in range(10):
        truth[np.arange(n_loci), 1, at[:, k]] = (truth[np.arange(n_loci), 0, at[:, k]] + 1 + k % 3) % 4
    win = truth[:, np.arange(members) % 2].transpose(1, 0, 2).copy()              # [member = read][locus][base]
    for _ in range(2):
        p = rng.integers(0, bases, size=win.shape[:2])
        r, l = np.meshgrid(np.arange(members), np.arange(n_loci), indexing="ij")
        win[r, l, p] = (win[r, l, p] + rng.integers(1, 4, size=p.shape)) % 4
    lens = bases - rng.integers(0, 4, size=win.shape[:2])
    keep = np.arange(bases)[None, None, :] < lens[:, :, None]
    off = np.zeros(members * n_loci + 1, np.int64)
    off[1:] = np.cumsum(lens.reshape(-1))
    read = np.repeat(np.arange(members, dtype=np.int32), n_loci)                  # rows ascending by (read, locus)
    locus = np.tile(np.arange(n_loci, dtype=np.int32), members)
    support_off = np.arange(n_loci + 1, dtype=np.int64) * members
    sup_read = np.tile(np.arange(members, dtype=np.int32), n_loci)
    return dict(read=read, locus=locus, win_off=off, win_bases=win[keep], support_off=support_off, sup_read=sup_read, value=np.full(members * n_loci, bases, np.int32)), lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--members", type=int, default=30)
    ap.add_argument("--bases", type=int, default=60)
    ap.add_argument("--max-dist", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--modes", default="four,one", help="four = four alignments per wavefront, one = MTR_TEST_SEQ_ROWS=0; under a kernel trace give one of them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_calls_probe.json"))
    args = ap.parse_args()
    case, lens = workload(args.loci, args.members, args.bases)
    K = args.max_dist
    diff = np.abs(lens[:, None, :] - lens[None, :, :])[np.triu_indices(args.members, 1)]
    width = diff + 2 * ((K - diff) >> 1) + 1
    buckets = [int(((width > lo) & (width <= hi)).sum()) for lo, hi in ((0, 32), (32, 64), (64, 128), (128, 256))]
    eng = mtr_amd.Engine()
    dev = torch.device("cuda", eng.device)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in case.items()}
    sg = SimpleNamespace(n_loci=args.loci, read=t["read"], locus=t["locus"])
    win = mtr_amd.GenotypeWindows(t["win_off"], t["win_bases"])
    calls = SimpleNamespace(support_off=t["support_off"], read=t["sup_read"], value=t["value"])
    modes = args.modes.split(",")
    times, outs = {mode: [] for mode in modes}, {}
    for _ in range(args.rounds):
        for mode in modes:
            if mode == "one":
                os.environ["MTR_TEST_SEQ_ROWS"] = "0"
            else:
                os.environ.pop("MTR_TEST_SEQ_ROWS", None)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            outs[mode] = eng.call_alleles_by_sequence(sg, win, calls, max_dist=K)
            torch.cuda.synchronize(dev)
            times[mode].append((time.perf_counter() - t0) * 1e3)
    first, last = outs[modes[0]], outs[modes[-1]]
    same = all(torch.equal(x, y) for x, y in zip((*first.calls, *first[1:]), (*last.calls, *last[1:])))
    zyg = first.calls.zygosity.cpu().numpy()
    row = dict(loci=args.loci, members=args.members, bases=args.bases, max_dist=K, pairs=int(first.dist.numel()), pairs_by_bucket=buckets, same_columns=same,
               zygosity_counts=[int((zyg == z).sum()) for z in (0, 1, 2)])
    for mode in times:
        ms = times[mode][1:] or times[mode]
        row.update({f"{mode}_ms_median": statistics.median(ms), f"{mode}_ms_min": min(ms), f"{mode}_ms_max": max(ms)})
    print(json.dumps(row), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="Engine.call_alleles_by_sequence whole, four alignments per wavefront against one (MTR_TEST_SEQ_ROWS=0)", rows=[row]), fh, indent=1)
        fh.write("\n")
    assert same


if __name__ == "__main__":
    main()
