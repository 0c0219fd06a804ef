"""Probe: the call time of Engine.window_structure on the GPU against the host's way of doing the same alignments.

    python tests/dev/gpu_window_structure.py [--out profiles/window_structure_probe.json] [--check PATH]

4 000 and 40 000 windows of 60 and 1 500 bases - copies of the structure's motifs with 5 % errors, cut to length - with ["CAG"] and with a
four-motif structure.  HTT's own four motifs, CAG CAACAG CCGCCA CCG, are 18 columns and beyond the limit of 16 for more than two motifs, so the
four-motif structure here is CAG CAA CCGCCA CCG: 15 columns, the same instantiation (<16, wide>) a user of four motifs gets.  The GPU figure is
the host clock around a synchronised window_structure call, whole: one warm-up, the median of five with min and max.  The yardstick is what a
user does without the call: the windows on the host and mtr_amd/csrc/window_structure.h run by ONE thread over the same windows
(tests/window_structure_check.cpp --time) - a lower bound of the host's way, not the GPU code under test.  --check names that program (built
with g++ -O2 when absent).  Both sides' scores are summed and must agree."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mtr_amd  # noqa: E402

STRUCTURES = (["CAG"], ["CAG", "CAA", "CCGCCA", "CCG"])
SHAPES = [(N, n) for N in (4000, 40000) for n in (60, 1500)]
RATE = 0.05


def windows(st, N, n, seed):
    """N windows of n bases: the motifs' copies in order (the first and the last motif share what the others leave), 5 % substitutions"""
    rng = np.random.default_rng(seed)
    code = lambda m: np.array(["ACGT".index(c) for c in m], np.uint8)      # noqa: E731
    mid = np.concatenate([code(m) for m in st[1:-1]] + [np.zeros(0, np.uint8)])
    out = np.empty((N, n), np.uint8)
    for w in range(N):
        a = int(rng.integers(1, max(2, (n - len(mid)) // len(st[0]))))
        row = np.concatenate([np.tile(code(st[0]), a), mid, np.tile(code(st[-1]), n // len(st[-1]) + 1)])[:n] if len(st) > 1 else np.tile(code(st[0]), n // len(st[0]) + 1)[:n]
        out[w] = row
    hit = rng.random((N, n)) < RATE
    out[hit] = rng.integers(0, 4, int(hit.sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_structure_probe.json"))
    ap.add_argument("--check", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    check = args.check
    if check is None or not os.path.exists(check):
        check = os.path.join(tmp, "window_structure_check")
        subprocess.run(["g++", "-std=c++17", "-O2", "-o", check, os.path.join(ROOT, "tests", "window_structure_check.cpp")], check=True)
    eng = mtr_amd.Engine()
    dev = torch.device("cuda", eng.device)
    rows = []
    for kind, st in enumerate(STRUCTURES):
        for N, n in SHAPES:
            y = windows(st, N, n, 10 * kind + N + n)
            path = os.path.join(tmp, "windows.bin")
            with open(path, "wb") as fh:
                fh.write(np.array([N, n, kind], np.int32).tobytes())
                fh.write(y.tobytes())
            host = json.loads(subprocess.run([check, "--time", path], check=True, stdout=subprocess.PIPE, text=True).stdout)
            off = torch.arange(N + 1, dtype=torch.int64, device=dev) * n
            bases, which = torch.from_numpy(y.reshape(-1)).to(dev), torch.zeros(N, dtype=torch.int32, device=dev)
            times = []
            for k in range(6):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                ws = eng.window_structure([st], off, bases, which)
                torch.cuda.synchronize(dev)
                times.append((time.perf_counter() - t0) * 1e3)
            times = times[1:]
            score_sum = int(ws.score.sum().item())
            assert score_sum == host["score_sum"] and not ws.skipped.any(), (score_sum, host)
            row = dict(structure=" ".join(st), windows=N, bases=n, gpu_ms_median=statistics.median(times), gpu_ms_min=min(times), gpu_ms_max=max(times),
                       host_ms=host["host_ms"], speedup=host["host_ms"] / statistics.median(times), score_sum=score_sum)
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    with open(args.out, "w") as fh:
        json.dump(dict(what="Engine.window_structure whole against one host thread running window_structure.h", rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
