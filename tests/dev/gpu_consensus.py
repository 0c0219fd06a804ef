"""Probe: the call time of Engine.allele_consensus on the GPU against the host's way of doing the same alignments.

    python tests/dev/gpu_consensus.py [--out profiles/consensus_probe.json] [--check PATH]

64 loci with two alleles each, 30 and 300 members per allele, windows of 60 and 1 500 bases (noisy copies of a random allele at 3 % errors),
band_extra 16.  The GPU figure is the host clock around a synchronised allele_consensus call (both passes: the size call and the writing call,
as the method makes them): one warm-up, the median of five with min and max.  The yardstick is what a user does without the call: the windows
on the host and mtr_amd/csrc/banded_align.h run by ONE thread over the same tasks (tests/banded_align_check.cpp --time: fill and vote walk, no
emission) - a lower bound of the host's way, not the GPU code under test.  --check names that program (built with g++ -O2 when absent).  The
largest shape's host time is measured on every eighth locus and scaled; the JSON says so."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mtr_amd  # noqa: E402
from tests import consensus_cases as cc  # noqa: E402
from tests import consensus_ref as ref  # noqa: E402

LOCI, EXTRA, RATE = 64, 16, 0.03


def noisy(truth, rng):
    """consensus_ref.noisy_read's model, vectorised"""
    n = len(truth)
    kind = np.where(rng.random(n) < RATE, rng.integers(3, size=n), -1)
    counts = np.where(kind == 2, 0, np.where(kind == 1, 2, 1))
    start = np.cumsum(counts) - counts
    out = np.repeat(truth, counts)
    sub, ins = kind == 0, kind == 1
    out[start[sub]] = (truth[sub] + 1 + rng.integers(3, size=int(sub.sum()))) % 4
    out[start[ins]] = rng.integers(4, size=int(ins.sum()))
    return out.astype(np.uint8)


def make_case(members, length, seed):
    rng = np.random.default_rng(seed)
    loci = []
    for _ in range(LOCI):
        alleles = []
        for _a in range(2):
            truth = cc.seq(rng, length)
            alleles.append(sorted((noisy(truth, rng) for _ in range(members)), key=len))
        loci.append((2, alleles[0], alleles[1]))
    return cc.build(loci, EXTRA, seed=seed, spare_rows=0)


def host_ms(case, check, every):
    tasks = []
    for A, al in enumerate(ref.alleles(case)):
        if al is not None and (A // 2) % every == 0:
            tasks += [(w, al[1]) for w in al[2]]
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(np.array([len(tasks), EXTRA], np.int64).tobytes())
        for w, b in tasks:
            f.write(np.array([len(w), len(b)], np.int32).tobytes() + w.tobytes() + b.tobytes())
    try:
        out = subprocess.run([check, "--time", f.name], capture_output=True, text=True, check=True).stdout
    finally:
        os.unlink(f.name)
    return float(out.split(":")[-1].split()[0]) * every, len(tasks), out.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_probe.json"))
    ap.add_argument("--check", default=os.path.join(tempfile.gettempdir(), "banded_align_check"))
    args = ap.parse_args()
    if not os.path.exists(args.check):
        subprocess.run(["g++", "-std=c++17", "-O2", "-o", args.check, os.path.join(ROOT, "tests", "banded_align_check.cpp")], check=True)
    eng = mtr_amd.Engine()
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    shapes = []
    for members, length in ((30, 60), (300, 60), (30, 1500), (300, 1500)):
        case = make_case(members, length, 7 * members + length)
        sg = SimpleNamespace(n_loci=case["n_loci"], read=t(case["read"]), locus=t(case["locus"]))
        win = mtr_amd.GenotypeWindows(t(case["win_off"]), t(case["win_bases"]))
        calls = SimpleNamespace(support_off=t(case["support_off"]), read=t(case["sup_read"]), allele=t(case["allele"]), zygosity=t(case["zygosity"]))
        times = []
        for k in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cons = eng.allele_consensus(sg, win, calls, band_extra=EXTRA)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times = times[1:]
        every = 8 if members * length >= 300 * 1500 else 1
        h_ms, h_tasks, h_line = host_ms(case, args.check, every)
        row = dict(loci=LOCI, members_per_allele=members, window=length, band_extra=EXTRA, tasks=int(cons.aligned.sum()), skipped=int(cons.skipped.sum()),
                   consensus_bases=int(cons.bases.numel()), gpu_call_ms_median=statistics.median(times), gpu_call_ms_min=min(times), gpu_call_ms_max=max(times),
                   host_one_thread_ms=h_ms, host_tasks_timed=h_tasks, host_scaled_by=every, host_output=h_line)
        print(json.dumps(row), flush=True)
        shapes.append(row)
    eng.close()
    doc = dict(what="Engine.allele_consensus: host clock around synchronised calls, 1 warm-up, median of 5 (min, max); the yardstick is banded_align.h on one host thread "
                    "over the same tasks (fill + vote walk, no emission, windows already on the host)", device=torch.cuda.get_device_name(dev), shapes=shapes)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
