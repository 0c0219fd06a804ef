#!/usr/bin/env python3
"""Development aid: where the wavefront-cycles of mtr_k_polish go, phase by phase, on the GPU.  Needs a library built with
-DMTR_PROFILE -DMTR_PROFILE_POLISH (mtr_amd/libmtr_hip_polprof.so; hipcc line: README, development tools; add -DMTR_POLISH_WALK_ALL for the
walk over every position).  Each phase has a spare counter of its own (device_util.hip.inc, wc_time_pol); the few counts that other kernels of
a profiling build add to the same spare counters (thousands, against 1e8 cycles and more) stay in the cycles.
    python3 tests/dev/polish_phases.py [reads] [workload] [seed]"""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("MTR_STAGED", "1")
os.environ.setdefault("MTR_LIB", os.path.join(ROOT, "mtr_amd", "libmtr_hip_polprof.so"))
import mtr_amd
from mtr_amd import synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
wl = sys.argv[2] if len(sys.argv) > 2 else "headline2k"
seed = int(sys.argv[3]) if len(sys.argv) > 3 else 2
reads = [c for _, c in synth.make_reads(wl, n, seed)]
eng = mtr_amd.Engine()
eng.upload(reads)
eng.run()
eng.run()
d = eng.counters()                # (a launch of the resident batch starts its counters from zero)
names = (("prof43", "queue pull and item loads"), ("prof44", "candidate in"), ("prof45", "staging and the flag test"),
         ("prof46", "table build"), ("prof47", "the walk"), ("prof55", "result out"))
tot = sum(d[k] for k, _ in names)
print(f"{wl}, {n} reads, seed {seed}: one launch ({os.path.basename(os.environ['MTR_LIB'])}); mtr_k_polish {tot / 1e9:.3f} G wave-cycles in its phases "
      f"(cyc_polish, the calls of polish() alone: {d['cyc_polish'] / 1e9:.3f} G)")
for k, label in names:
    print(f"  {label:28s} {d[k] / 1e9:8.3f} G cycles {100.0 * d[k] / max(tot, 1):5.1f} %")
moved = d["prof44"] + d["prof47"] + d["prof55"]
print(f"  candidate in + walk + result out: {moved / 1e9:.3f} G")
print(json.dumps({"workload": wl, "reads": n, "seed": seed, "lib": os.path.basename(os.environ["MTR_LIB"]),
                  "phases": {k: d[k] for k, _ in names}, "cyc_polish": d["cyc_polish"], "kmer_tables": d.get("kmer_tables"), "kmer_lookups": d.get("kmer_lookups")}))
eng.close()
