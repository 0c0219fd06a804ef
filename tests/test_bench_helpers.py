"""bench.py's CPU-side helpers: the committed PMC profiles are read per workload, the slot-time summary adds up, the known answers and inputs that the
command-line legs of the driver's line compare with exist."""
import json
import os

import bench
from tests import golden_util as gu


def test_committed_profiles_belong_to_their_workloads():
    for cfg, name in ((None, "pmc_latest.json"), ("c3", "pmc_c3.json")):
        with open(os.path.join(bench.ROOT, "profiles", name)) as fh:
            raw = json.load(fh)
        assert raw["config"] == (cfg or "headline2k")
        prof, tag = bench.profiled_counters(cfg)
        if prof is None:                                         # the kernel sources moved on since the profile: the line then carries nulls, by design
            assert tag.startswith("stale") and raw["kernel_src_sha"] != bench.kernel_sources_sha()
            continue
        st = bench.slot_time(prof)
        assert abs(sum(prof["chain_per_launch"][k].get("wave_cycles", 0.0) for k in prof["chain_per_launch"]) - st["sum_wave_cycles"]) < 1.0
        assert 0 < st["service_kernels_wave_cycles"] < st["sum_wave_cycles"]
        assert abs(st["ms_on_4096_slots_at_2.4GHz"] - st["sum_wave_cycles"] / (4096 * 2.4e9) * 1e3) < 1e-9
    assert bench.profiled_counters("c2")[0] is None              # no profile of config 2: its line says null, not the headline's numbers


def test_known_answers_of_the_command_line_legs_exist():
    for f in ("c2_1000_stdout.json", "c4_100000_stdout.json", "c2_1000_wire.json", "c3_100_wire.json", "c4_100k_wire.json",
              "headline2k_10000_wire.json", "headline2k_10000_p_wire.json", "headline2k_10000_stdout.json", "headline2k_10000_p_stdout.json",
              "c4_10000_stdout.json"):
        with open(os.path.join(gu.GOLDEN, f)) as fh:
            k = json.load(fh)
        assert len(k["sha256"]) == 64
    assert len(bench.C5_FILES) == 15
    for n in bench.C5_FILES:
        assert os.path.exists(gu.input_path(n)) and os.path.exists(os.path.join(gu.GOLDEN, f"{n}.p.stdout"))


def _known_answers_with_inputs():
    out = []
    for f in sorted(os.listdir(gu.GOLDEN)):
        if f.endswith(("_wire.json", "_stdout.json")):
            with open(os.path.join(gu.GOLDEN, f)) as fh:
                k = json.load(fh)
            if "input_sha256" in k:
                out.append((f, k))
    return out


def test_known_answers_still_describe_the_reads_synth_makes():
    """A known answer is the answer for the reads mtr_amd.synth made when it was written: regenerate the inputs of every fixture that
    records their hash (input_sha256 = sha256 of the concatenated base codes) and check it - a change to synth must come with new fixtures."""
    import hashlib

    from mtr_amd import synth
    known = _known_answers_with_inputs()
    names = {f for f, _ in known}
    assert {"headline2k_10000_wire.json", "headline2k_10000_p_wire.json", "headline2k_10000_stdout.json", "headline2k_10000_p_stdout.json",
            "c4_10000_stdout.json"} <= names, names
    made = {}
    for f, k in known:
        key = (k["config"], k["n_reads"], k["seed"])
        if key not in made:
            reads = synth.make_reads(*key)
            h = hashlib.sha256()
            for _, codes in reads:
                h.update(codes.astype("uint8").tobytes())
            made[key] = (h.hexdigest(), sum(len(c) for _, c in reads))
        assert k["seed"] == synth.CONFIGS[k["config"]][4], f
        assert made[key][0] == k["input_sha256"], f"{f}: mtr_amd.synth no longer makes the reads this known answer describes"
        if "sum_len" in k:
            assert made[key][1] == k["sum_len"], f
        if "chunk_sha256" in k:
            assert len(k["chunk_sha256"]) == -(-k["n_reads"] // k["chunk_reads"]), f


def test_headline_known_answers_agree_with_the_oracle_on_their_first_chunk():
    """the first chunk_sha256 of each headline wire fixture is the CPU oracle's wire form of reads 0..499 as it stands (the whole fixture takes
    ~130 core-seconds; tests/golden/make_c4_wire_hash.py)"""
    import hashlib

    from mtr_amd import synth
    from tests.host_util import load_known, wire_record
    from tests.oracle_binding import Oracle
    reads = [c for _, c in synth.make_reads("headline2k", 500, 2)]
    for name, manhattan in (("headline2k_10000_wire.json", True), ("headline2k_10000_p_wire.json", False)):
        k = load_known(name)
        orc = Oracle(manhattan=manhattan)
        blob = b"".join(wire_record(r) for c in reads for r in orc.process(c))
        orc.close()
        assert k["chunk_reads"] == 500 and hashlib.sha256(blob).hexdigest() == k["chunk_sha256"][0], name


def test_known_wire_mismatch_names_the_first_bad_chunk_and_read():
    """the GPU tests' diagnosis of a failing whole-stream comparison (tests/host_util.known_wire_mismatch), on oracle records with one
    field of one read changed"""
    import hashlib

    from mtr_amd import synth
    from tests import host_util as hu
    from tests.oracle_binding import Oracle
    reads = [c for _, c in synth.make_reads("c2", 40, 5)]
    orc = Oracle()
    recs = [orc.process(c) for c in reads]
    orc.close()
    per_read = [b"".join(hu.wire_record(r) for r in rs) for rs in recs]
    assert [hu.wire_tuples(b) for b in per_read] == recs
    counts = [len(rs) for rs in recs]
    blob = b"".join(per_read)
    assert hu.wire_split(blob, counts) == per_read
    known = {"n_reads": 40, "records": sum(counts), "wire_bytes": len(blob), "sha256": hashlib.sha256(blob).hexdigest(), "chunk_reads": 10,
             "chunk_sha256": [hashlib.sha256(b"".join(per_read[i:i + 10])).hexdigest() for i in range(0, 40, 10)]}
    msg = lambda i, want, got: f"read {i}: {want == got}"          # noqa: E731
    assert hu.known_wire_mismatch(blob, counts, reads, known, msg) is None
    bad = next(i for i in range(23, 40) if counts[i])
    rec = list(recs[bad][0])
    rec[6] += 1                                                     # num_mismatches
    blob2 = b"".join(per_read[:bad]) + hu.wire_record(rec) + per_read[bad][len(hu.wire_record(rec)):] + b"".join(per_read[bad + 1:])
    got = hu.known_wire_mismatch(blob2, counts, reads, known, msg)
    assert got is not None and f"first bad chunk {bad // 10} " in got and got.endswith(f"read {bad}: False"), got
    assert "does not parse" in hu.known_wire_mismatch(blob[:-4], counts, reads, known, msg)


def _wire_of_golden_records(name="synth_c2", mode="default"):
    """the reference's records of a golden case (G4), packed to the wire form by the library's own mtr_pack_records (host code, no GPU)"""
    import ctypes as C

    import mtr_amd
    from mtr_amd import build as mbuild

    mbuild.build()
    lib = mtr_amd.load_library()
    per_read = [[gu.g4_tuple(ev) for ev in rd["G4"]] for rd in gu.capture_by_read(name, mode)]
    flat = [r for rs in per_read for r in rs]
    recs = (mtr_amd.CRecord * len(flat))()
    for c, r in zip(recs, flat):
        for f, v in zip(bench.RECORD_FIELDS, r[:13]):
            setattr(c, f, v)
        c.unit = r[13].encode()
        c.unit_score[:len(r[14])] = r[14]
    cap = sum(56 + ((r[3] + 3) & ~3) + 4 * r[3] for r in flat)
    buf = C.create_string_buffer(cap)
    assert lib.mtr_pack_records(recs, len(flat), buf, cap) == cap
    return buf.raw, per_read


def test_decode_wire_returns_the_packed_records():
    blob, per_read = _wire_of_golden_records()
    flat = [r for rs in per_read for r in rs]
    fields, units, scores = bench.decode_wire(blob, len(flat))
    assert [tuple(int(x) for x in row) for row in fields] == [r[:13] for r in flat]
    assert units.tobytes().decode() == "".join(r[13] for r in flat)
    assert scores.tolist() == [s for r in flat for s in r[14]]


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_above_the_cap(tmp_path):
    import numpy as np

    blob, per_read = _wire_of_golden_records()
    flat = [r for rs in per_read for r in rs]
    counts = np.array([len(rs) for rs in per_read], np.int32)
    full = bench.dump_outputs(str(tmp_path / "full"), [blob], [len(flat)], counts)
    assert full["sampled"] is None and full["records"] == len(flat)
    got = {f[:-4]: np.load(tmp_path / "full" / f) for f in os.listdir(tmp_path / "full")}
    assert set(got) == {"records", "units", "unit_scores", "records_per_read"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["records"].tolist() == [list(r[:13]) for r in flat] and got["records_per_read"].tolist() == counts.tolist()
    assert "".join(map(chr, got["units"].astype(int))) == "".join(r[13] for r in flat)
    assert sum(v.nbytes for v in got.values()) == full["bytes"]
    cap = full["bytes"] // 3                                     # a third of the output: the same seeded sample of reads every time, within the cap
    a = bench.dump_outputs(str(tmp_path / "a"), [blob], [len(flat)], counts, cap_bytes=cap)
    b = bench.dump_outputs(str(tmp_path / "b"), [blob], [len(flat)], counts, cap_bytes=cap)
    assert a["sampled"] == "reads" and 0 < a["bytes"] <= cap and a["files"] == b["files"]
    keep = np.load(tmp_path / "a" / "sample_index.npy").astype(int)
    assert np.array_equal(keep, np.load(tmp_path / "b" / "sample_index.npy"))
    want = [list(r[:13]) for i in keep for r in per_read[i]]
    assert np.load(tmp_path / "a" / "records.npy").tolist() == want
    assert np.load(tmp_path / "a" / "records_per_read.npy").tolist() == counts[keep].tolist()
    # without per-read counts (the N > 1 exchange) the sample is one of records
    c = bench.dump_outputs(str(tmp_path / "c"), [blob[:len(blob)], b""], [len(flat), 0], cap_bytes=cap)
    assert c["sampled"] == "records" and c["bytes"] <= cap and not os.path.exists(tmp_path / "c" / "records_per_read.npy")
