"""Stage-level parity of the unit phase on the GPU (-m gpu): what the kernels compute INSIDE a range, against capture
points of the unmodified reference (tests/golden), so that a regression in the walks or the revision is localised and
does not only show up as "record differs":
  G2   search_De_Bruijn_graph (consensus.c:507-582): per (window, k) the found flag and the unit chosen among the two walk
       directions with its alignment  <-> trace event 2;
  G3p  polish_repeat (consensus.c:610-704): unit in / unit out                                  <-> trace event 4;
  G3r  revise_representative_unit_sub (consensus.c:851-1046): unit in, scores, revised unit     <-> trace event 5.
The same stage by stage in the staged chain (what every product path runs), and - against the CPU oracle, which answers for any
(read, window, k) - every search and every single walk (trace event 8) on a seeded set that reaches all four k-mer table layouts.
Units are compared through their length and an FNV-1a checksum of their base codes (what the trace carries).
Plus the builder-side sweeps promoted into the suite: BASELINE config 2 at 1 000 reads and the config-3 shape at 16 reads,
every read against the oracle; -a on a config-3-shaped read through the command line; the accuracy table of
test_single_TR/test.sh on 200 reads per unit length."""
import collections
import gzip
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import mtr_amd
from mtr_amd import synth
from tests import golden_util as gu
from tests import unit_search_set as uss
from tests.test_gpu_parity import MODES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = {"A": 0, "C": 1, "G": 2, "T": 3}


def fnv(unit: str) -> int:
    h = 2166136261
    for ch in unit:
        h = ((h ^ LUT[ch]) * 16777619) & 0xFFFFFFFF
    return h & 0x7FFFFFFF


def traced_run(name, mask):
    os.environ["MTR_STAGED"] = "0"                         # the per-read kernel: the reference's own order of ranges (the sequential loop)
    os.environ["MTR_TRACE_MASK"] = str(mask)
    try:
        e = mtr_amd.Engine()
        reads = gu.read_fasta(gu.input_path(name))
        e.set_trace(2_000_000)
        e.upload([c for _, c in reads])
        e.run()
        ev = e.get_trace()
        e.close()
    finally:
        del os.environ["MTR_STAGED"], os.environ["MTR_TRACE_MASK"]
    assert len(ev) < 2_000_000
    return ev


@pytest.mark.parametrize("name", ["3_5", "synth_2k"])
def test_search_stage_matches_reference_G2(name):
    ev = traced_run(name, 1 << 2)
    got = {}
    for e in ev[ev[:, 0] == 2]:
        rd, qs, qe, k, found = int(e[1]), int(e[2]), int(e[3]), int(e[4]), int(e[5])
        got.setdefault((rd, qs, qe, k), []).append((found, tuple(int(x) for x in e[7:16])))
    n = 0
    with gzip.open(os.path.join(gu.GOLDEN, f"{name}.default.l2.jsonl.gz"), "rt") as fh:
        for line in fh:
            g = json.loads(line)
            key = (g["rd"], g["qs"], g["qe"], g["k"])
            assert key in got, f"the GPU never searched {key}"
            founds = [f for f, _ in got[key]]
            assert g["found"] in founds, (key, g["found"], founds)
            if g["found"]:
                want = (g["period"], g["rep_start"], g["rep_end"], g["repeat_len"], g["copies"], g["mat"], g["mis"], g["ins"], g["del"])
                assert any(f == 1 and v == want for f, v in got[key]), (key, want, got[key])
                n += 1
    assert n > 20


STAGE_MODES = ["per_read", "staged", "staged_quads", "staged_two_pass"]


def traced_run_in_mode(monkeypatch, mode, reads, mask, cap):
    """the trace of one launch in an arrangement of tests/test_gpu_parity.py's MODES; a chain mode must have run as the chain, every read in it"""
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MTR_TRACE_MASK", str(mask))
    e = mtr_amd.Engine()
    try:
        e.set_trace(cap)
        e.upload(list(reads))
        e.run()
        ev = e.get_trace()
        if mode == "per_read":
            assert e.last_mode() == "per-read kernel"
        else:
            assert e.last_mode() == "staged chain"
            assert e.counters()["reads_sent_back"] == 0
    finally:
        e.close()
    assert len(ev) < cap, "the trace filled"
    return ev


@pytest.mark.parametrize("name", ["synth_2k", "synth_c2", "10_50", "20_50"])
def test_polish_and_revision_stages_match_reference_G3p_G3r(name):
    ev = traced_run(name, (1 << 4) | (1 << 5))
    cap = gu.capture_by_read(name, "default")
    n_p = n_r = 0
    for rd, per_read in enumerate(cap):
        mine = ev[ev[:, 1] == rd]
        # polish: one call per revision, in the reference's order
        got_p = [(int(e[2]), int(e[3]), int(e[4]), int(e[5]), int(e[6]), int(e[7])) for e in mine[mine[:, 0] == 4]]
        want_p = [(g["rep_start"], g["rep_end"], g["k"], len(g["in"]), len(g["out"]), fnv(g["out"])) for g in per_read["G3p"]]
        assert got_p == want_p, f"{name} read {rd}: polish_repeat calls differ"
        n_p += len(want_p)
        # revision rounds: the kernel answers a round it has already run from its memo, so it runs a subset of the
        # reference's calls - every one it runs must be one of the reference's, and every distinct one of the reference's
        # must have been run
        got_r = {(int(e[2]), int(e[3]), int(e[4]), int(e[5]), int(e[6]), int(e[7]), int(e[8]), int(e[9])) for e in mine[mine[:, 0] == 5]}
        want_r = {(g["rep_start"], g["rep_end"], len(g["in"]), g["G"], g["MM"], g["D"], g["out_period"],
                   fnv(g["out"]) if 0 < g["out_period"] < 1024 else 0) for g in per_read["G3r"]}
        assert got_r == want_r, f"{name} read {rd}: revise_representative_unit_sub results differ: {sorted(got_r ^ want_r)[:4]}"
        n_r += len(want_r)
    assert n_p > 0 and n_r > 0


@pytest.mark.parametrize("mode", STAGE_MODES[1:])
@pytest.mark.parametrize("name", ["synth_2k", "synth_c2", "10_50", "20_50"])
def test_polish_and_revision_stages_in_the_chain_match_reference_G3p_G3r(monkeypatch, name, mode):
    """The test above in the staged chain.  The per-read kernel keeps the reference's own order of ranges, so there the polish calls compare
    as ordered lists; the chain searches ranges in any order, and also ranges the reference never reaches (an earlier record had removed them): per read every golden polish call and every
    golden revision result must be there (the polish calls with their multiplicity), and whatever else the GPU ran may only concern an
    alignment that is none of the read's recorded repeats (capture point G4)."""
    reads = [c for _, c in gu.read_fasta(gu.input_path(name))]
    ev = traced_run_in_mode(monkeypatch, mode, reads, (1 << 4) | (1 << 5), 2_000_000)
    cap = gu.capture_by_read(name, "default")
    n_p = n_r = extras = 0
    for rd, per_read in enumerate(cap):
        mine = ev[ev[:, 1] == rd]
        got_p = collections.Counter((int(e[2]), int(e[3]), int(e[4]), int(e[5]), int(e[6]), int(e[7])) for e in mine[mine[:, 0] == 4])
        want_p = collections.Counter((g["rep_start"], g["rep_end"], g["k"], len(g["in"]), len(g["out"]), fnv(g["out"])) for g in per_read["G3p"])
        got_r = collections.Counter((int(e[2]), int(e[3]), int(e[4]), int(e[5]), int(e[6]), int(e[7]), int(e[8]), int(e[9])) for e in mine[mine[:, 0] == 5])
        want_r = {(g["rep_start"], g["rep_end"], len(g["in"]), g["G"], g["MM"], g["D"], g["out_period"],
                   fnv(g["out"]) if 0 < g["out_period"] < 1024 else 0) for g in per_read["G3r"]}
        recorded = {(g["rep_start"], g["rep_end"]) for g in per_read["G4"]}
        missing_p = want_p - got_p
        assert not missing_p, f"{name} [{mode}] read {rd}: polish_repeat calls of the reference missing: {sorted(missing_p)[:4]}"
        missing_r = want_r - set(got_r)
        assert not missing_r, f"{name} [{mode}] read {rd}: revise_representative_unit_sub results of the reference missing: {sorted(missing_r)[:4]}"
        extra = list((got_p - want_p).elements()) + [r for r in got_r.elements() if r not in want_r]
        bad = [x for x in extra if (x[0], x[1]) in recorded]
        assert not bad, f"{name} [{mode}] read {rd}: {len(bad)} of {len(extra)} events beyond the reference's concern a recorded repeat: {bad[:4]}"
        extras += len(extra)
        n_p += sum(want_p.values())
        n_r += len(want_r)
    print(f"{name} [{mode}]: {n_p} polish calls, {n_r} revision results, {extras} events beyond the reference's")
    assert n_p > 0 and n_r > 0, f"{extras} events beyond the reference's"


# ---- every search and every walk against the CPU oracle, in every arrangement -------------------------------------------------------------------
_SEARCH, _WALK = {}, {}                     # the oracle's answers, shared by the modes: (set, rd, qs, qe, k) / (set, rd, qs, qe, k, backward, seed)
_CLEARED = (-1,) * 9


def _oracle_search(oracle, which, reads, key):
    if (which, *key) not in _SEARCH:
        _SEARCH[(which, *key)] = oracle.search_unit(reads[key[0]], key[1], key[2], key[3])
    return _SEARCH[(which, *key)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", STAGE_MODES)
@pytest.mark.parametrize("which", ["small", "wide"])
def test_every_search_and_every_walk_matches_the_oracle(monkeypatch, which, mode):
    """Trace events 2 (one per searched (window, k)) and 8 (one per walk) of tests/unit_search_set.py's reads - `wide`: the two long reads, in a run of
    their own - against mtro_search_unit and mtro_walk:
      * every event 2 the GPU emitted - also those of ranges the reference's loop never reaches, and every occurrence of a key - has the oracle's found
        flag; where found, its nine fields; where not, the cleared record: that is what find_tandem_repeat_sub makes of it (handle_one_read.c:84).  (The
        reference's own record may then still hold the forward walk's alignment, SURVEY H4 - capture point G2 shows it, nobody reads it, and the kernels
        do not align it.)
      * every (window, k) of the oracle's level-3 capture was searched; in per_read mode the GPU searches nothing else.  (Where the smaller k's bound
        the node count to five the kernels answer without building the table, k2_range_walks: the event then says so - not found, the cleared record -
        and the oracle must agree like for any other.)
      * every event 8 has the period of the oracle's walk from that seed in that direction (0: it did not close).  Steps are not compared: the kernels'
        cycle check ends a walk that cannot close before the reference's loop does.
    The shares of closed walks among the events 8 are printed per layout.  Each of the four layouts must have some in the `small` run; the `wide` run is
    there for the tables in global memory, and must have closed walks of k <= 6 in the window wider than 65535 (the oracle finds units there)."""
    from tests.oracle_binding import Oracle
    reads = uss.small_reads() if which == "small" else uss.wide_reads()
    events = uss.oracle_g2_small() if which == "small" else uss.oracle_g2_wide()
    if which == "small":
        uss.assert_every_regime_is_reached(uss.oracle_g2_small() + uss.oracle_g2_wide())
    t0 = time.time()
    ev = traced_run_in_mode(monkeypatch, mode, reads, (1 << 2) | (1 << 8), 4_000_000)
    t_gpu = time.time() - t0
    oracle = Oracle()
    try:
        # ---- event 2
        e2 = np.unique(ev[ev[:, 0] == 2][:, [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15]], axis=0)
        searched = set()
        n_found = 0
        for row in e2.tolist():
            key, found, fields = tuple(row[:4]), row[4], tuple(row[5:])
            searched.add(key)
            want = _oracle_search(oracle, which, reads, key)
            assert found == want["found"], (mode, key, found, want)
            want_fields = tuple(want[f] for f in uss.FIELDS) if want["found"] else _CLEARED
            assert fields == want_fields, (mode, key, fields, want)
            n_found += found
        captured = {(g["rd"], g["qs"], g["qe"], g["k"]) for g in events}
        missing = captured - searched
        assert not missing, f"[{mode}] the GPU never searched {len(missing)} of the oracle's {len(captured)} (window, k): {sorted(missing)[:4]}"
        if mode == "per_read":
            assert searched == captured, sorted(searched - captured)[:4]
        assert n_found >= sum(g["found"] for g in events) > 40
        # ---- event 8
        e8 = np.unique(ev[ev[:, 0] == 8][:, [1, 2, 3, 4, 5, 6, 8]], axis=0)
        share = {name: [0, 0] for name in uss.LAYOUTS}
        closed_wide_low_k = 0
        for rd, qs, qe, k, backward, seed, period in e8.tolist():
            wkey = (which, rd, qs, qe, k, backward, seed)
            if wkey not in _WALK:
                _WALK[wkey] = oracle.walk(reads[rd], qs, qe, k, bool(backward), seed)[0]
            assert period == _WALK[wkey], (mode, wkey, period, _WALK[wkey])
            s = share[uss.layout(qe - qs + 1, k)]
            s[0] += period > 0
            s[1] += 1
            closed_wide_low_k += period > 0 and qe - qs + 1 > 65535 and k <= 6
    finally:
        oracle.close()
    print(f"{which} [{mode}]: GPU run {t_gpu:.2f} s, whole test {time.time() - t0:.2f} s; {len(e2)} searches ({n_found} found), "
          f"{len(e8)} walks; closed walks per layout: " + ", ".join(f"{n} {c}/{t}" for n, (c, t) in share.items()))
    for name in (uss.LAYOUTS if which == "small" else ("split_global",)):
        assert share[name][0] > 0, (name, share)
    if which == "wide":
        assert closed_wide_low_k > 0, share


def _oracle_chunk(args):
    reads, manhattan = args
    from tests.oracle_binding import Oracle
    o = Oracle(manhattan=manhattan)
    out = [o.process(c) for c in reads]
    o.close()
    return out


def _against_oracle(reads, manhattan=True, workers=8):
    chunks = [reads[i::workers] for i in range(workers)]
    with ProcessPoolExecutor(workers) as ex:
        parts = list(ex.map(_oracle_chunk, [(c, manhattan) for c in chunks]))
    want = [None] * len(reads)
    for w, part in enumerate(parts):
        want[w::workers] = part
    e = mtr_amd.Engine(manhattan=manhattan)
    got = e.process(reads)
    e.close()
    return [i for i in range(len(reads)) if [tuple(r) for r in got[i]] != want[i]]


@pytest.mark.timeout(900)
def test_config2_at_full_size_every_read_against_the_oracle():
    """BASELINE config 2: 1 000 reads, unit 100 x 10 copies, L ~ 1.25 kb"""
    reads = [c for _, c in synth.make_reads("c2")]
    assert len(reads) == 1000
    assert _against_oracle(reads) == []


@pytest.mark.timeout(900)
def test_config3_shape_16_reads_against_the_oracle():
    """BASELINE config 3 shape: unit 200 x 200 copies, L ~ 42 kb (DPs of 4 M cells)"""
    reads = [c for _, c in synth.make_reads("c3", 16, 3)]
    assert _against_oracle(reads) == []


@pytest.mark.timeout(900)
def test_config3_at_full_size_record_stream_is_the_oracles():
    """BASELINE config 3 as bench.py measures it (its --full line's secondary.c3 runs the same child): 100 reads of unit 200 x 200 copies,
    the launch's record stream in wire form against the CPU oracle's known answer (tests/golden/c3_100_wire.json)."""
    import json
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("MTR_LIB", "RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--config", "c3", "--steps", "1", "--warmup", "1", "--no-cli", "--no-latency", "--cpu-sample", "0"],
                       capture_output=True, env=env, timeout=800, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-800:]
    line = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert line["matches_oracle"] is True and line["record_stream"]["records"] == 1724, line.get("record_stream")
    assert "config 3" in line["metric"] and line["config"]["reads_per_gpu"] == 100


@pytest.mark.timeout(900)
def test_bench_without_full_runs_only_the_headline(tmp_path):
    """bench.py without --full: set-up, warm-up, timed steps, --dump-outputs and the line - none of the legs or checks --full adds"""
    env = {k: v for k, v in os.environ.items() if k not in ("MTR_LIB", "RANK", "WORLD_SIZE", "LOCAL_RANK")}
    dump = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--reads", "2000", "--dump-outputs", str(dump)],
                       capture_output=True, env=env, timeout=800, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode()[-800:]
    line = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert line["unit"] == "reads/s" and line["higher_is_better"] is True and line["dtype"] == "int32" and line["steps"] == 3 and line["warmup"] == 1
    assert abs(line["value"] - 2000 / (line["ms_per_step"] / 1e3)) < 1e-6 * line["value"]          # reads per second of the timed steps
    full_only = {"reference_work_per_launch", "roofline", "value_kernel", "value_with_upload", "boundary", "latency_ms_per_read_p50", "value_cli", "cli",
                 "launcher", "value_launcher", "launcher_rccl_forced", "baseline_configs_cli", "host_ceiling", "cpu_baseline", "secondary"}
    assert not full_only & set(line), sorted(full_only & set(line))
    assert line["chain_health"]["ok"] is True
    recs = np.load(dump / "records.npy")
    assert recs.shape == (line["dumped_outputs"]["records"], 13) and len(recs) > 0
    assert np.load(dump / "records_per_read.npy").shape == (2000,)


@pytest.mark.timeout(900)
def test_cli_alignments_on_a_config3_shaped_read(tmp_path):
    from tests.oracle_binding import ORACLE_DIR
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "mtr_amd", "host"), "mTR"], check=True)
    fa = tmp_path / "c3.fa"
    synth.write_fasta(str(fa), synth.make_reads("c3", 2, 7))
    want = subprocess.run([os.path.join(ORACLE_DIR, "mtr_oracle_cli"), "-a", str(fa)], capture_output=True, check=True).stdout
    p = subprocess.run([os.path.join(ROOT, "mtr_amd", "host", "mTR"), "-a", str(fa)], capture_output=True)
    assert p.returncode == 0, p.stderr.decode()[:500]
    assert p.stdout == want and len(want) > 100000


@pytest.mark.timeout(900)
def test_accuracy_table_equals_the_oracles(tmp_path):
    """test_single_TR/test.sh:35-63 with count_match / comp_mTR_DP (tools/accuracy.py, tools/unit_score.c): unit lengths
    2..200 x 10 copies, 200 seeded reads each.  The GPU driver's report must score exactly as the oracle CLI's report on the
    same files (it is the same report), and the predictions must be good: the table is an accuracy harness, not only a diff."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import accuracy
    from tests.oracle_binding import ORACLE_DIR
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "mtr_amd", "host"), "mTR"], check=True)
    lib = accuracy.load_scorer()
    for u in (2, 5, 10, 20, 50, 100, 200):
        rng = np.random.RandomState(1000 + u)
        reads, truth = [], []
        for i in range(200):
            codes, unit = synth.make_read(rng, u, 10, u * 10, u * 10)
            reads.append((str(i), codes))
            truth.append("".join("ACGT"[int(x)] for x in unit))
        fa = tmp_path / f"u{u}.fa"
        synth.write_fasta(str(fa), reads)
        gpu = subprocess.run([os.path.join(ROOT, "mtr_amd", "host", "mTR"), str(fa)], capture_output=True, check=True).stdout.decode()
        orc = subprocess.run([os.path.join(ORACLE_DIR, "mtr_oracle_cli"), str(fa)], capture_output=True, check=True).stdout.decode()
        sg, so = accuracy.score(lib, gpu, truth), accuracy.score(lib, orc, truth)
        assert sg == so and gpu == orc, u
        assert sg["report_lines"] >= 150, (u, sg)
        assert sg["ratio>=0.94"] >= 0.8 * len(reads), (u, sg)               # the reference's own level on this error profile (90-100 %)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("profile", ["sub_heavy", "sub_del"])
def test_the_references_other_error_profiles_against_the_oracle(profile):
    """test_single_TR/test.sh:12-18 carries two alternates to the Nanopore profile (substitution 12.7 / insertion 3.2 / deletion 4.7 %
    and 9.7 / 2.9 / 7.5 %): substitution-heavy reads give a different mix of DPs, revisions and memo hits.  300 reads of each shape
    (the headline's unit 100 x 10 and mixed units 50-200), every read against the oracle, in the chain with and without the
    four-per-wavefront passes."""
    prof = synth.PROFILES[profile]
    reads = [c for _, c in synth.make_reads("headline2k", 150, 41, prof)] + [c for _, c in synth.make_reads("c4", 150, 42, prof)]
    assert _against_oracle(reads) == []
    os.environ["MTR_QUAD_MIN"] = "1"
    try:
        assert _against_oracle(reads) == []
    finally:
        del os.environ["MTR_QUAD_MIN"]
