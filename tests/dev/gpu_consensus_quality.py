"""Probe: what the quality weights cost - Engine.allele_consensus_quality against Engine.allele_consensus, and the quality gather of a FASTQ upload
against the same upload without it.

    python tests/dev/gpu_consensus_quality.py [--out profiles/consensus_quality_probe.json]

The shapes are tests/dev/gpu_consensus.py's: 64 loci with two alleles each, 30 and 300 members per allele, windows of 60 and 1 500 bases, band_extra
16; qualities seeded 0 .. 60, qual_cap 40.  Both calls come from the same library in the same process and are ALTERNATED: one warm-up of each, then
five rounds of (unweighted, weighted), the host clock around each synchronised call (both passes: the size call and the writing call, as the
methods make them); the median of five with min and max.  The yardstick is the unweighted call, which the weights do not touch.
The upload: a FASTQ file of 24 MiB (reads of 8 000 bases) in device memory, upload_fastq_device with keep_quality off and on, alternated the same
way; the difference is the gather (one offset scan, one kernel, one synchronisation)."""
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
from gpu_consensus import EXTRA, LOCI, make_case  # noqa: E402

CAP, ROUNDS = 40, 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(prefix, times):
    return {f"{prefix}_ms_median": statistics.median(times), f"{prefix}_ms_min": min(times), f"{prefix}_ms_max": max(times)}


def fastq_file(n_bytes, read_len, seed):
    rng = np.random.default_rng(seed)
    rec = 14 + 2 * read_len                                  # "@read0000\n" bases "\n+\n" qualities "\n"
    n = n_bytes // rec
    out = np.empty((n, rec), np.uint8)
    out[:, :10] = np.frombuffer(b"@read0000\n", np.uint8)
    out[:, 10:10 + read_len] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, read_len))]
    out[:, 10 + read_len:13 + read_len] = np.frombuffer(b"\n+\n", np.uint8)
    out[:, 13 + read_len:13 + 2 * read_len] = rng.integers(33, 74, size=(n, read_len))
    out[:, 13 + 2 * read_len] = 10
    return out.reshape(-1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_quality_probe.json"))
    args = ap.parse_args()
    eng = mtr_amd.Engine()
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    shapes = []
    for members, length in ((30, 60), (300, 60), (30, 1500), (300, 1500)):
        case = make_case(members, length, 7 * members + length)
        qual = t(np.random.default_rng(members + length).integers(0, 61, size=len(case["win_bases"])).astype(np.uint8))
        sg = SimpleNamespace(n_loci=case["n_loci"], read=t(case["read"]), locus=t(case["locus"]))
        win = mtr_amd.GenotypeWindows(t(case["win_off"]), t(case["win_bases"]))
        calls = SimpleNamespace(support_off=t(case["support_off"]), read=t(case["sup_read"]), allele=t(case["allele"]), zygosity=t(case["zygosity"]))
        plain = lambda: eng.allele_consensus(sg, win, calls, band_extra=EXTRA)                                       # noqa: E731
        weighted = lambda: eng.allele_consensus_quality(sg, win, qual, calls, band_extra=EXTRA, qual_cap=CAP)      # noqa: E731
        plain(), weighted()
        tp, tw = [], []
        for _ in range(ROUNDS):
            ms, cons = timed(plain)
            tp.append(ms)
            ms, consq = timed(weighted)
            tw.append(ms)
        row = dict(loci=LOCI, members_per_allele=members, window=length, band_extra=EXTRA, qual_cap=CAP, tasks=int(cons.aligned.sum()), consensus_bases=int(cons.bases.numel()),
                   weighted_consensus_bases=int(consq.bases.numel()), **stats("unweighted_call", tp), **stats("weighted_call", tw))
        row["weighted_over_unweighted"] = row["weighted_call_ms_median"] / row["unweighted_call_ms_median"]
        print(json.dumps(row), flush=True)
        shapes.append(row)
    data, n_reads = fastq_file(24 << 20, 8000, 5)
    buf = t(data)
    up = lambda keep: (lambda: eng.upload_fastq_device(buf, keep_quality=keep))      # noqa: E731
    up(False)(), up(True)()
    off, on = [], []
    for _ in range(ROUNDS):
        off.append(timed(up(False))[0])
        on.append(timed(up(True))[0])
    upload = dict(file_bytes=int(buf.numel()), reads=n_reads, read_bases=8000, quality_bytes=eng.qualities_resident(), **stats("upload", off), **stats("upload_keep_quality", on))
    upload["gather_ms_by_difference"] = upload["upload_keep_quality_ms_median"] - upload["upload_ms_median"]
    print(json.dumps(upload), flush=True)
    eng.close()
    doc = dict(what="Engine.allele_consensus_quality against Engine.allele_consensus, alternated in one process: host clock around synchronised calls, 1 warm-up, median of 5 "
                    "(min, max); and upload_fastq_device of a 24 MiB file with keep_quality off and on, the same way", device=torch.cuda.get_device_name(dev), shapes=shapes,
               upload=upload)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
