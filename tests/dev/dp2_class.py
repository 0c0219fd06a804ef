#!/usr/bin/env python3
"""Development aid: the forward passes of mtr_k_dp2_quads by columns per lane (DPQ_COLS class), on the GPU.  Needs a library built with
-DMTR_PROFILE -DMTR_PROFILE_DP2_CLASS (mtr_amd/libmtr_hip_dp2cls.so; hipcc line: README, development tools).  A spare counter per class holds the
forward-pass cycles in its low 44 bits and the number of passes above them (k3_staged.hip.inc st_quad_run); the few counts that other kernels of a
profiling build add to the same spare counters (thousands, against 1e9 cycles) stay in the cycles.
    python3 tests/dev/dp2_class.py [reads] [workload] [seed]"""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("MTR_STAGED", "1")
os.environ.setdefault("MTR_LIB", os.path.join(ROOT, "mtr_amd", "libmtr_hip_dp2cls.so"))
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
names = (("prof43", "1 column per lane, units <= 8"), ("prof44", "1 column per lane, units 9-16"), ("prof45", "2 columns per lane (units 17-32)"),
         ("prof46", "3-6 columns per lane (units 33-96)"), ("prof47", "7-8 columns per lane (units 97-128)"))
MASK = (1 << 44) - 1
cyc = {k: d[k] & MASK for k, _ in names}
cnt = {k: d[k] >> 44 for k, _ in names}
tot_c, tot_n = sum(cyc.values()), sum(cnt.values())
print(f"{wl}, {n} reads, seed {seed}: one launch; mtr_k_dp2_quads forward passes {tot_n}, {tot_c / 1e9:.3f} G wave-cycles "
      f"(cyc_dp_fwd of the launch {d['cyc_dp_fwd'] / 1e9:.3f} G, cyc_dp_tb {d['cyc_dp_tb'] / 1e9:.3f} G)")
for k, label in names:
    print(f"  {label:38s} {cnt[k]:9d} passes {100.0 * cnt[k] / max(tot_n, 1):5.1f} %   {cyc[k] / 1e9:8.3f} G cycles {100.0 * cyc[k] / max(tot_c, 1):5.1f} %   "
          f"{cyc[k] / max(cnt[k], 1):8.0f} cycles a pass")
print(json.dumps({"workload": wl, "reads": n, "seed": seed, "cycles": cyc, "passes": cnt, "cyc_dp_fwd": d["cyc_dp_fwd"], "cyc_dp_tb": d["cyc_dp_tb"],
                  "qpass_bytes_dp2": d["qpass_bytes_dp2"], "qpass_cells_dp2": d["qpass_cells_dp2"]}))
eng.close()
