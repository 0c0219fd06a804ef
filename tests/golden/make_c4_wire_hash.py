#!/usr/bin/env python3
"""Known answer for BASELINE config 4 at full size: sha256 of the record tables (wire form of include/mtr_hip.h, read
after read in input order) that the CPU ORACLE (oracle/mtr_oracle.c, pinned to the reference) produces for the 100 000
mixed-unit reads of mtr_amd.synth config "c4" (seed 4).  bench.py --strong c4 compares the stream gathered from the N
ranks with it: the multi-GPU result must be bit-identical to the reference's, whatever N.

  python tests/golden/make_c4_wire_hash.py [-j 6]      -> tests/golden/c4_100k_wire.json   (~3 min on 6 cores)
  python tests/golden/make_c4_wire_hash.py --config c3 -n 100   -> tests/golden/c3_100_wire.json (config 3's shape: 100 reads of 42 kb)
  python tests/golden/make_c4_wire_hash.py --config headline2k -n 10000 [--pearson]
      -> tests/golden/headline2k_10000_wire.json / headline2k_10000_p_wire.json (the bench's headline batch; ~25 s on 6 cores)

The headline fixtures also carry chunk_sha256 (one hash per job of 500 reads, in input order: a failing GPU test names
the first bad chunk from it) and input_sha256 (sha256 of the concatenated base codes of all reads: a change to
mtr_amd/synth.py that alters the reads is caught on the CPU, tests/test_bench_helpers.py).
"""
import argparse
import hashlib
import json
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CHUNK = {"c3": 2, "c2": 100}          # reads per job; every other config: 500


def work(args):
    lo, hi, manhattan = args
    from tests.host_util import wire_record
    from tests.oracle_binding import Oracle
    reads = READS[lo:hi]
    orc = Oracle(manhattan=manhattan)
    out, nrec = [], 0
    for _, codes in reads:
        recs = orc.process(codes)
        nrec += len(recs)
        out.append(b"".join(wire_record(r) for r in recs))
    orc.close()
    return lo, b"".join(out), nrec


def input_sha256(reads) -> str:
    """sha256 of the base codes (0..3, one byte each) of all reads, concatenated in input order"""
    h = hashlib.sha256()
    for _, codes in reads:
        h.update(codes.astype("uint8").tobytes())
    return h.hexdigest()


def main():
    global READS
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=6)
    ap.add_argument("-n", type=int, default=100000)
    ap.add_argument("--config", default="c4", help="c4 (seed 4); c3 = BASELINE config 3's shape, seed 3 (bench.py's secondary.c3: -n 100); "
                                                    "headline2k = the bench's headline batch (seed 2: -n 10000)")
    ap.add_argument("--pearson", action="store_true", help="Pearson distance (mTR -p) instead of Manhattan")
    ap.add_argument("--made-by", default="", help="appended to made_by (e.g. how the fixture was cross-checked against the reference)")
    a = ap.parse_args()
    assert 1 <= a.j <= 8, "size the oracle pool at 8 processes or fewer"
    from mtr_amd import synth
    seed = synth.CONFIGS[a.config][4]          # (c4: 4, c3: 3, c2: 1, headline2k: 2)
    READS = synth.make_reads(a.config, a.n, seed)
    step = CHUNK.get(a.config, 500)
    jobs = [(lo, min(lo + step, a.n), not a.pearson) for lo in range(0, a.n, step)]
    h = hashlib.sha256()
    chunks = []
    total_bytes = total_rec = 0
    with mp.get_context("fork").Pool(a.j) as pool:
        for lo, blob, nrec in pool.imap(work, jobs):          # imap keeps input order
            h.update(blob)
            chunks.append(hashlib.sha256(blob).hexdigest())
            total_bytes += len(blob)
            total_rec += nrec
    out = {"config": a.config, "seed": seed, "n_reads": a.n, "records": total_rec, "wire_bytes": total_bytes, "sha256": h.hexdigest(),
           "sum_len": int(sum(len(c) for _, c in READS)), "made_by": "tests/golden/make_c4_wire_hash.py (CPU oracle)" + (f"; {a.made_by}" if a.made_by else "")}
    new_style = a.config == "headline2k"        # the older fixtures keep their fields (they are not regenerated)
    if a.pearson or new_style:
        out.update({"pearson": bool(a.pearson), "chunk_reads": step, "chunk_sha256": chunks, "input_sha256": input_sha256(READS)})
    name = "c4_100k_wire.json" if (a.n == 100000 and a.config == "c4" and not a.pearson) else f"{a.config}_{a.n}{'_p' if a.pearson else ''}_wire.json"
    path = os.path.join(ROOT, "tests", "golden", name)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "chunk_sha256"}))


if __name__ == "__main__":
    main()
