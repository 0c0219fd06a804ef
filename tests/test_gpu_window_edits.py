"""The window edits on the MI355X (mtr_window_edits_device, mtr_window_edits_copy_device, Engine.window_edits, the kernels of
mtr_amd/csrc/window_edits.hip.inc).

Truth is tests/window_edits_ref.py, the definition of include/mtr_hip.h ("window edits") in plain Python; tests/test_window_edits_ref.py holds it
to hand-worked answers.  Everything is exact equality: every column, every dtype, every shape.  The inputs are tests/window_edits_cases.py's: the
window structure's (widths 1, 7, 8, 9, 15, 16, 17, 31, 32 with S <= 2 and 8, 9, 16 with S = 3, 4; every residue of 16; 130 windows of 130
structures; 0, 1, 63, 64, 65, 257 windows) and every length 0 .. 33 in every bin (a stored row is whole words: the rows have no packing boundary
of their own).  Every test here calls Engine.window_edits or the entry points behind it."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import consensus_cases as cc
from tests import window_edits_cases as ec
from tests import window_edits_ref as ref
from tests import window_structure_cases as wc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", eng.device))


def _args(eng, case):
    return case["structures"], _dev(eng, case["off"]), _dev(eng, case["bases"]), _dev(eng, case["which"])


def _run(eng, case, scores=(1, 1, 1)):
    return eng.window_edits(*_args(eng, case), *scores)


def _assert_we(got, want, what=""):
    for name, g, w in zip(mtr_amd.WindowEdits._fields, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        g = g.cpu()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not torch.equal(g, w):
            at = (g != w).nonzero()[0].tolist()
            raise AssertionError((what, name, at, g[tuple(at)].item(), w[tuple(at)].item()))


def _assert_invariants(case, got, what):
    """per window and segment, from the device's own columns: copies * U == matches + subs + dels, end - start == matches + subs + ins"""
    off, edits, seg = got.off.cpu().numpy(), got.edits.cpu().numpy(), got.seg.cpu().numpy().astype(np.int64)
    N = len(case["which"])
    U = np.zeros((N, 4), np.int64)
    for w, k in enumerate(case["which"]):
        st = case["structures"][k]
        st = [st] if isinstance(st, str) else st
        U[w, :len(st)] = [len(m) for m in st]
    kinds = np.zeros((N, 4, 3), np.int64)
    np.add.at(kinds, (np.repeat(np.arange(N), np.diff(off)), edits[:, 1], edits[:, 4]), 1)
    assert (seg[:, :, 2] * U == seg[:, :, 3] + kinds[:, :, 0] + kinds[:, :, 2]).all(), what
    assert (seg[:, :, 1] - seg[:, :, 0] == seg[:, :, 3] + kinds[:, :, 0] + kinds[:, :, 1]).all(), what


@pytest.mark.parametrize("scores", ec.SCORES)
@pytest.mark.parametrize("name", ["widths", "lengths", "residues"] + [f"count{N}" for N in ec.COUNTS])
def test_every_column_equals_the_reference(eng, name, scores):
    case, want = ec.expected()[(name, scores)]
    got = _run(eng, case, scores)
    _assert_we(got, want, (name, scores))
    _assert_invariants(case, got, (name, scores))
    ws = eng.window_structure(*_args(eng, case), *scores)
    assert torch.equal(got.seg, ws.seg) and torch.equal(got.score, ws.score) and torch.equal(got.skipped, ws.skipped), name
    again = _run(eng, case, scores)
    assert all(torch.equal(x, y) for x, y in zip(got, again)), name


@pytest.mark.parametrize("scores", ec.SCORES)
def test_130_windows_of_130_structures_in_one_launch(eng, scores):
    """every lane carries its own structure: a kernel that took lane 0's would fail here"""
    case, want = ec.expected()[("lanes", scores)]
    got = _run(eng, case, scores)
    _assert_we(got, want, ("lanes", scores))
    _assert_invariants(case, got, ("lanes", scores))


def test_the_hand_worked_interruption_on_the_device(eng):
    case = wc.case([["CAG"]], [np.array(ref._codes("CAG" * 10 + "CAA" + "CAG" * 9), np.uint8), np.array(ref._codes("CAGCAGAGCAG"), np.uint8)], [0, 0])
    got = _run(eng, case)
    assert got.off.cpu().tolist() == [0, 1, 2] and got.edits.cpu().tolist() == [[32, 0, 10, 2, 0, 0], [6, 0, 2, 0, 2, 1]]
    assert got.score.cpu().tolist() == [58, 10]


def test_the_longest_window_and_one_beyond_it(eng):
    n = mtr_amd.WS_MAX_WINDOW
    longest, beyond = np.zeros(n, np.uint8), np.zeros(n + 1, np.uint8)
    longest[9000] = beyond[9000] = 1
    case = wc.case(["A"], [longest, beyond, np.array([0, 1, 0], np.uint8)], [0, 0, 0])
    got = _run(eng, case)
    assert got.skipped.cpu().tolist() == [0, 1, 0] and got.score.cpu().tolist() == [n - 2, 0, 1] and got.off.cpu().tolist() == [0, 1, 1, 2]
    assert got.edits.cpu().tolist() == [[9000, 0, 9000, 0, 0, 1], [1, 0, 1, 0, 0, 1]]
    assert got.seg[0].cpu().tolist() == [[0, n, n, n - 1]] + [[0] * 4] * 3 and got.seg[1].cpu().tolist() == [[0] * 4] * 4
    ws = eng.window_structure(*_args(eng, case))
    assert torch.equal(got.seg, ws.seg) and torch.equal(got.score, ws.score) and torch.equal(got.skipped, ws.skipped)


def test_several_rounds_give_the_tensors_of_one(eng, monkeypatch):
    case, want = ec.expected()[("count257", (1, 1, 1))]
    one = _run(eng, case)
    few = eng.test_window_edits_rounds()
    monkeypatch.setenv("MTR_TEST_WE_SCRATCH_BYTES", "4")            # below any group's slot: every group is a round of its own
    many = _run(eng, case)
    rounds = eng.test_window_edits_rounds()
    monkeypatch.delenv("MTR_TEST_WE_SCRATCH_BYTES")
    assert few == 1 and rounds >= 3, (few, rounds)                   # both bins' groups side by side in one round by default; every group of 64 windows a round of its own under the knob
    _assert_we(many, want, "several rounds")
    assert all(torch.equal(x, y) for x, y in zip(one, many))


def test_structures_beyond_the_limits_are_refused(eng):
    one = wc.case(["A"], [np.zeros(4, np.uint8)], [0])
    for st, words in ((["A" * 33], "1 motifs of 33 bases"), (["A" * 16, "C" * 17], "2 motifs of 33 bases"), (["A" * 15, "C", "G"], "3 motifs of 17 bases"),
                      (["A"] * 5, "5 motifs outside 1..4"), ([], "0 motifs outside 1..4"), (["A", ""], "motif 1: length 0"), (["AC", "AN"], "motif 1: byte 78 at 1")):
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: structure 1.*" + words):
            eng.window_edits(["A", st], _dev(eng, one["off"]), _dev(eng, one["bases"]), _dev(eng, one["which"]))
    full = wc.case([["A" * 16, "C" * 16], ["ACGT"] * 4], [np.zeros(4, np.uint8)] * 2, [0, 1])          # at the limits: taken
    _assert_we(_run(eng, full), ref.columns(full["structures"], full["windows"], full["which"]), "at the limits")


def test_the_refusals_write_nothing_and_the_next_call_succeeds(eng):
    case, want = ec.expected()[("count65", (1, 1, 1))]
    N, T, E = len(case["which"]), len(case["bases"]), len(want[1])
    dev = torch.device("cuda", eng.device)
    off, bases, which = _dev(eng, case["off"]), _dev(eng, case["bases"]), _dev(eng, case["which"])
    cols = [torch.full(s, 77, dtype=t, device=dev) for s, t in (((N + 1,), torch.int64), ((E, 6), torch.int32), ((N, 4, 4), torch.int32), ((N,), torch.int32), ((N,), torch.uint8))]
    ptrs = [c.data_ptr() for c in cols]
    motifs = [m.encode() for st in case["structures"] for m in st]
    data = np.frombuffer(b"".join(motifs), np.uint8).copy()
    moff = np.concatenate([[0], np.cumsum([len(m) for m in motifs])]).astype(np.int64)
    soff = np.concatenate([[0], np.cumsum([len(st) for st in case["structures"]])]).astype(np.int32)
    K = len(case["structures"])
    n_edits = C.c_int64(-1)

    def compute(off=off, bases=bases, which=which, scores=(1, 1, 1), n_structs=K, n_bases=T, host=(data, moff, soff), out=C.byref(n_edits)):
        st = eng.lib.mtr_window_edits_device(eng.h, host[0].ctypes.data, host[1].ctypes.data, host[2].ctypes.data, n_structs, off.data_ptr(), bases.data_ptr(),
                                             which.data_ptr(), N, n_bases, *scores, None, out)
        return mtr_amd.STATUS[st], eng.lib.mtr_last_error(eng.h).decode()

    def copy(cap_windows=N, cap_edits=E, dst_ptrs=ptrs):
        dst = mtr_amd.CWindowEditsDst(*dst_ptrs, cap_windows, cap_edits)
        st = eng.lib.mtr_window_edits_copy_device(eng.h, C.byref(dst))
        return mtr_amd.STATUS[st], eng.lib.mtr_last_error(eng.h).decode()

    torch.cuda.synchronize()
    bad_off = case["off"].copy()
    bad_off[[5, 6]] = bad_off[[6, 5]] if bad_off[5] != bad_off[6] else (bad_off[5] + 1, bad_off[6])
    bad_which = case["which"].copy()
    bad_which[9] = K
    bad_bases = case["bases"].copy()
    bad_bases[11], bad_bases[40] = 4, 200
    moff_down = moff.copy()
    moff_down[2] = moff_down[1] - 1
    for kw, words in ((dict(scores=(6, 1, 1)), "gain = 6"), (dict(scores=(1, 0, 1)), "mismatch = 0"), (dict(scores=(1, 1, 4)), "indel = 4"), (dict(n_structs=0), "n_structs = 0"),
                      (dict(host=(data, moff_down, soff)), "motif_off decreases at motif 1"), (dict(out=None), "NULL"),
                      (dict(off=_dev(eng, bad_off)), "win_off at window 5 does not ascend"), (dict(n_bases=T - 1), "does not ascend from 0 to n_bases"),
                      (dict(which=_dev(eng, bad_which)), f"window 9: win_struct {K} outside 0..{K - 1}"),
                      (dict(bases=_dev(eng, bad_bases)), "win_bases at 11: code 4 is above 3"),
                      (dict(off=torch.from_numpy(case["off"])), "win_off is not device memory")):
        got = compute(**kw)
        assert got[0] == "MTR_ERR_BAD_ARG" and words in got[1], (kw.keys(), got)
        kept = copy()                                                                                  # a refused call keeps nothing to copy
        assert kept[0] == "MTR_ERR_BAD_ARG" and "no edits kept" in kept[1], (kw.keys(), kept)
        assert all((c == 77).all() for c in cols), kw.keys()
    assert compute()[0] == "MTR_OK" and n_edits.value == E
    for kw, words in ((dict(cap_edits=E - 1), f"destination holds {E - 1} edits, {E} needed"), (dict(cap_windows=N - 1), f"destination holds {N - 1} windows, {N} needed")):
        got = copy(**kw)
        assert got[0] == "MTR_ERR_OVERFLOW" and words in got[1], (kw, got)
        assert all((c == 77).all() for c in cols), kw
    got = copy(dst_ptrs=[ptrs[0], ptrs[1], None, ptrs[3], ptrs[4]])
    assert got[0] == "MTR_ERR_BAD_ARG" and "NULL" in got[1] and all((c == 77).all() for c in cols)
    assert copy()[0] == "MTR_OK"
    _assert_we(cols, want, "after the refusals")


# ---- from reads to the interruption of each called allele -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (2, 3))
def test_from_reads_to_the_one_substitution_of_each_allele(eng, seed):
    reads, loci = cc.truth_reads(seed), cc.truth_loci()
    eng.upload(reads)
    sg = eng.genotype_catalog(loci, 1)
    win = eng.genotype_windows(sg)
    calls = eng.call_alleles(sg, "bases")
    cons = eng.allele_consensus(sg, win, calls, band_extra=cc.TRUTH_EXTRA)
    alleles = torch.arange(2 * len(loci), dtype=torch.int32, device=cons.off.device) // 2
    we = eng.window_edits(["CAG", "GAA"], cons.off, cons.bases, alleles)
    # both alleles of the first locus carry a CAA: (CAG)10 CAA (CAG)9 and (CAG)25 CAA (CAG)6; the second locus is not called
    assert we.off.cpu().tolist() == [0, 1, 2, 2, 2] and we.edits.cpu().tolist() == [[32, 0, 10, 2, 0, 0], [77, 0, 25, 2, 0, 0]]
    assert we.score.cpu().tolist() == [58, 94, 0, 0] and we.seg[:2, 0].cpu().tolist() == [[0, 60, 20, 59], [0, 96, 32, 95]] and not we.skipped.any()
    ws = eng.window_structure(["CAG", "GAA"], cons.off, cons.bases, alleles)
    assert torch.equal(we.seg, ws.seg) and torch.equal(we.score, ws.score) and torch.equal(we.skipped, ws.skipped)
    text = mtr_amd.format_window_edits(["CAG"] * 2 + ["GAA"] * 2, we, names=["a0", "a1", "b0", "b1"])
    assert text == b"a0\t1\tCAG#10:2G>A@32\na1\t1\tCAG#25:2G>A@77\nb0\t0\nb1\t0\n"
    # the single reads: equal to the reference (a noisy read's edits need not be the truth's)
    per_read = eng.window_edits(["CAG", "GAA"], win.off, win.bases, sg.locus)
    off, bases = win.off.cpu().numpy(), win.bases.cpu().numpy()
    windows = [bases[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    _assert_we(per_read, ref.columns([["CAG"], ["GAA"]], windows, sg.locus.cpu().tolist()), "per read")
