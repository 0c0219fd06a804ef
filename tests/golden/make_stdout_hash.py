#!/usr/bin/env python3
"""Known answers for the command line on whole BASELINE configs: sha256 (and line count) of the stdout the CPU ORACLE's command line (oracle/mtr_oracle_cli,
pinned to the reference: same report lines as reference mTR run one read per process) prints for the reads of a mtr_amd.synth config written by
synth.write_fasta (IDs = the decimal read index).  bench.py's secondary.c2 / secondary.c4 compare `mTR -g N <fasta>`'s stdout with them: the multi-GPU
product path must print what the reference prints, whatever N.

  python tests/golden/make_stdout_hash.py c4 100000 [-j 7]     -> tests/golden/c4_100000_stdout.json   (~6 min on 7 cores)
  python tests/golden/make_stdout_hash.py c2 1000              -> tests/golden/c2_1000_stdout.json
  python tests/golden/make_stdout_hash.py c4 10000             -> tests/golden/c4_10000_stdout.json   (tests/test_gpu_multi.py's RCCL test)
  python tests/golden/make_stdout_hash.py headline2k 10000 [-p] -> tests/golden/headline2k_10000[_p]_stdout.json

input_sha256 (sha256 of the concatenated base codes of all reads) lets a CPU test see that mtr_amd.synth still makes the reads the
known answer describes.  --made-by appends a note (e.g. the cross-check against the reference run one read per process).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("n", type=int)
    ap.add_argument("-j", type=int, default=7)
    ap.add_argument("-p", action="store_true", help="Pearson distance (-p)")
    ap.add_argument("--made-by", default="", help="appended to made_by")
    a = ap.parse_args()
    from mtr_amd import synth
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle"], check=True)
    cli = os.path.join(ROOT, "oracle", "mtr_oracle_cli")
    assert 1 <= a.j <= 8, "size the oracle pool at 8 processes or fewer"
    seed = synth.CONFIGS[a.config][4]
    reads = synth.make_reads(a.config, a.n, seed)
    hin = hashlib.sha256()
    for _, codes in reads:
        hin.update(codes.astype("uint8").tobytes())
    h = hashlib.sha256()
    lines = total = 0
    with tempfile.TemporaryDirectory() as td:
        per = max(1, (a.n + 8 * a.j - 1) // (8 * a.j))
        shards = []
        for lo in range(0, a.n, per):
            f = os.path.join(td, f"s{lo}.fa")
            synth.write_fasta(f, reads[lo:lo + per])
            shards.append(f)
        # isolated semantics: a read's lines do not depend on its neighbours, so the shards' outputs in order are the whole file's output
        running = []
        nxt = 0
        outs = {}
        while nxt < len(shards) or running:
            while nxt < len(shards) and len(running) < a.j:
                o = open(shards[nxt] + ".out", "wb")
                running.append((nxt, subprocess.Popen([cli] + (["-p"] if a.p else []) + [shards[nxt]], stdout=o, stderr=subprocess.DEVNULL), o))
                nxt += 1
            i, p, o = running.pop(0)
            assert p.wait() == 0
            o.close()
            outs[i] = shards[i] + ".out"
        for i in range(len(shards)):
            b = open(outs[i], "rb").read()
            h.update(b)
            lines += b.count(b"\n")
            total += len(b)
    out = {"config": a.config, "seed": seed, "n_reads": a.n, "pearson": bool(a.p), "stdout_lines": lines, "stdout_bytes": total, "sha256": h.hexdigest(),
           "input_sha256": hin.hexdigest(),
           "made_by": "tests/golden/make_stdout_hash.py (oracle/mtr_oracle_cli on the FASTA of synth.write_fasta)" + (f"; {a.made_by}" if a.made_by else "")}
    path = os.path.join(ROOT, "tests", "golden", f"{a.config}_{a.n}{'_p' if a.p else ''}_stdout.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(path, out)


if __name__ == "__main__":
    main()
