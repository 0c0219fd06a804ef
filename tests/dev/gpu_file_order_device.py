#!/usr/bin/env python3
"""Development aid (GPU box): what file-order mode costs an upload from device memory.  The batch is bench.py's headline batch,
10 000 synthetic 2 kb reads, each cut by 0..199 bases so that most reads follow a longer one and find a tail.  Wall times, host clock
around calls that return synchronised (every upload ends with a stream synchronise); after warm-up, median and min..max of the repeats:
  device in file   upload_device(text, offsets, lens, file_state=FileState())
  via the host     text.cpu() -> reads -> upload(reads, FileState()): the only way to the same batch without the device state
  device isolated  upload_device(text, offsets, lens): the path that must not change
and the device time of mtr_k_file_tail alone (HIP events around the launch; id 0 of the kernel times after test_file_tail()).
usage: gpu_file_order_device.py [n_reads] [repeats] [json_out]"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import mtr_amd
from mtr_amd import synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
WARM = 3

rng = np.random.RandomState(11)
reads = [c[:len(c) - int(rng.randint(0, 200))] for _, c in synth.make_reads("headline2k", n, seed=2)]
lens = np.array([len(c) for c in reads], np.int32)
offs = np.cumsum(lens, dtype=np.int64) - lens
ascii_ = np.frombuffer(b"ACGT", np.uint8)[np.concatenate(reads)]
text = torch.from_numpy(ascii_).cuda()
lut = np.zeros(256, np.uint8)
lut[list(b"ACGT")] = [0, 1, 2, 3]
eng = mtr_amd.Engine()


def device_in_file():
    fs = mtr_amd.FileState()
    eng.upload_device(text, offs, lens, file_state=fs)
    fs.close()


def via_host():
    codes = lut[text.cpu().numpy()]
    fs = mtr_amd.FileState()
    eng.upload([codes[o:o + l] for o, l in zip(offs, lens)], fs)
    fs.close()


def device_isolated():
    eng.upload_device(text, offs, lens)


def timed(fn):
    ms = []
    for k in range(WARM + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms[WARM:])
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "repeats": reps}


out = {"n_reads": n, "bases": int(lens.sum()), "warmup": WARM}
# the two ways must give the same batch before their times mean anything
via_host()
want = eng.test_file_tail()
kernel_ms = []
for k in range(WARM + reps):
    device_in_file()
    got = eng.test_file_tail()
    kernel_ms.append(eng.kernel_times_ms()["k1_ranges"])               # id 0: mtr_k_file_tail after test_file_tail()
assert all(np.array_equal(a, b) for a, b in zip(got, want)), "device and host state disagree"
kernel_ms = np.array(kernel_ms[WARM:])
out["tail_entries"] = int(want[1][-1])
out["reads_with_a_tail"] = int((np.diff(want[1]) > 0).sum())
out["tail_kernel"] = {"median_ms": float(np.median(kernel_ms)), "min_ms": float(kernel_ms.min()), "max_ms": float(kernel_ms.max()), "repeats": reps}
out["device_in_file"] = timed(device_in_file)
out["via_host"] = timed(via_host)
out["device_isolated"] = timed(device_isolated)
try:
    out["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
except OSError:
    out["commit"] = None
line = json.dumps(out)
print(line, flush=True)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as fh:
        fh.write(line + "\n")
eng.close()
