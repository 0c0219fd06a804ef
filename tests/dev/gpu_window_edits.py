"""Probe: the call time of Engine.window_edits on the GPU against Engine.window_structure on the same windows, and against the host's way of
listing the same edits.

    python tests/dev/gpu_window_edits.py [--out profiles/window_edits_probe.json] [--check PATH]

The four shapes and two structures of tests/dev/gpu_window_structure.py (its windows() makes them).  Both GPU figures are the host clock around a
synchronised call, whole: one warm-up, the median of five with min and max.  The yardsticks are window_structure's own call time - what the
stored decisions, the two walks and the list cost on top of the rows - and ONE host thread running mtr_amd/csrc/window_edits.h over the same
windows (tests/window_edits_check.cpp --time: rows, counting walk, emitting walk), a lower bound of the host's way.  Neither is the code under
test.  --check names that program (built with g++ -O2 when absent).  Both sides' edit counts must agree, and the rounds the call took are
recorded."""
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
from tests.dev.gpu_window_structure import SHAPES, STRUCTURES, windows  # noqa: E402


def timed(dev, call):
    times = []
    for _ in range(6):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize(dev)
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_edits_probe.json"))
    ap.add_argument("--check", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    check = args.check
    if check is None or not os.path.exists(check):
        check = os.path.join(tmp, "window_edits_check")
        subprocess.run(["g++", "-std=c++17", "-O2", "-o", check, os.path.join(ROOT, "tests", "window_edits_check.cpp")], check=True)
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
            ws, ws_ms = timed(dev, lambda: eng.window_structure([st], off, bases, which))
            we, we_ms = timed(dev, lambda: eng.window_edits([st], off, bases, which))
            edits = int(we.edits.shape[0])
            assert edits == host["edit_sum"] and torch.equal(we.seg, ws.seg) and torch.equal(we.score, ws.score), (edits, host)
            row = dict(structure=" ".join(st), windows=N, bases=n, rounds=eng.test_window_edits_rounds(), edits=edits,
                       edits_ms_median=statistics.median(we_ms), edits_ms_min=min(we_ms), edits_ms_max=max(we_ms),
                       structure_ms_median=statistics.median(ws_ms), structure_ms_min=min(ws_ms), structure_ms_max=max(ws_ms),
                       over_structure=statistics.median(we_ms) / statistics.median(ws_ms), host_ms=host["host_ms"], speedup=host["host_ms"] / statistics.median(we_ms))
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    with open(args.out, "w") as fh:
        json.dump(dict(what="Engine.window_edits whole against Engine.window_structure whole and one host thread running window_edits.h", rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
