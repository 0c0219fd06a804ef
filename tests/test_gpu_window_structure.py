"""The window structure on the MI355X (mtr_window_structure_device, Engine.window_structure, with_segment_copies, the kernels of
mtr_amd/csrc/window_structure.hip.inc).

Truth is tests/window_structure_ref.py, the definition of include/mtr_hip.h in plain Python; tests/test_window_structure_ref.py holds it to
hand-worked answers and shows that the inputs of tests/window_structure_cases.py are not degenerate.  Everything is exact equality: every
column, every dtype, every shape, ratio as float32 bits."""
import ctypes as C

import numpy as np
import pytest

import mtr_amd
from tests import consensus_cases as cc
from tests import window_structure_cases as wc
from tests import window_structure_ref as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mtr_amd.Engine()
    yield e
    e.close()


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", eng.device))


def _run(eng, case, scores=(1, 1, 1)):
    return eng.window_structure(case["structures"], _dev(eng, case["off"]), _dev(eng, case["bases"]), _dev(eng, case["which"]), *scores)


def _assert_ws(got, want, what=""):
    for name, g, w in zip(mtr_amd.WindowStructure._fields, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        g = g.cpu()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if name == "ratio":
            g, w = g.view(torch.int32), w.view(torch.int32)
        if not torch.equal(g, w):
            at = (g != w).nonzero()[0].tolist()
            raise AssertionError((what, name, at, g[tuple(at)].item(), w[tuple(at)].item()))


@pytest.mark.parametrize("scores", wc.SCORES)
@pytest.mark.parametrize("name", ["widths", "residues"] + [f"count{N}" for N in wc.COUNTS])
def test_every_column_equals_the_reference(eng, name, scores):
    case, want = wc.expected()[(name, scores)]
    got = _run(eng, case, scores)
    _assert_ws(got, want, (name, scores))
    again = _run(eng, case, scores)
    assert all(torch.equal(x, y) for x, y in zip(got, again)), name


@pytest.mark.parametrize("scores", wc.SCORES)
def test_130_windows_of_130_structures_in_one_launch(eng, scores):
    """every lane carries its own structure: a kernel that took lane 0's would fail here"""
    case, want = wc.expected()[("lanes", scores)]
    _assert_ws(_run(eng, case, scores), want, ("lanes", scores))


def test_the_wraps_left_and_the_ties_on_the_device(eng):
    """the hand-worked windows: CAGCAGAGCAG takes the wrap's left (sweep 2), (CAG)5 C (CCG)3 a sub that ties up"""
    for window, st, scores, score, segs in wc.HAND:
        case = wc.case([st], [np.array(ref.codes(window), np.uint8)], [0])
        got = _run(eng, case, scores)
        assert got.score.cpu().tolist() == [score] and got.seg[0, :len(st)].cpu().tolist() == [list(s) for s in segs], (window, st, scores, got.seg.cpu().tolist())
        _assert_ws(got, ref.columns([st], case["windows"], [0], *scores), (window, st))


def test_the_longest_window_and_one_beyond_it(eng):
    n = mtr_amd.WS_MAX_WINDOW
    case = wc.case(["A", ["A", "C"]], [np.zeros(n, np.uint8), np.zeros(n + 1, np.uint8), np.zeros(3, np.uint8)], [0, 0, 1])
    got = _run(eng, case)
    assert got.skipped.cpu().tolist() == [0, 1, 0] and got.score.cpu().tolist() == [n, 0, 3]
    assert got.seg[0].cpu().tolist() == [[0, n, n, n]] + [[0] * 4] * 3 and got.seg[1].cpu().tolist() == [[0] * 4] * 4
    assert got.seg[2].cpu().tolist() == [[0, 3, 3, 3], [3, 3, 0, 0], [0] * 4, [0] * 4]
    assert got.ratio.cpu().tolist() == [1.0, 0.0, 1.0]


def test_structures_beyond_the_limits_are_refused(eng):
    one = wc.case(["A"], [np.zeros(4, np.uint8)], [0])
    for st, words in ((["A" * 33], "1 motifs of 33 bases"), (["A" * 16, "C" * 17], "2 motifs of 33 bases"), (["A" * 15, "C", "G"], "3 motifs of 17 bases"),
                      (["A"] * 5, "5 motifs outside 1..4"), ([], "0 motifs outside 1..4"), (["A", ""], "motif 1: length 0"), (["AC", "AN"], "motif 1: byte 78 at 1")):
        with pytest.raises(mtr_amd.MtrError, match="MTR_ERR_BAD_ARG: structure 1.*" + words):
            eng.window_structure(["A", st], _dev(eng, one["off"]), _dev(eng, one["bases"]), _dev(eng, one["which"]))
    full = wc.case([["A" * 16, "C" * 16], ["ACGT"] * 4], [np.zeros(4, np.uint8)] * 2, [0, 1])          # at the limits: taken
    _assert_ws(_run(eng, full), ref.columns(full["structures"], full["windows"], full["which"]), "at the limits")


def test_the_refusals_write_nothing_and_the_next_call_succeeds(eng):
    case, want = wc.expected()[("count65", (1, 1, 1))]
    N, T = len(case["which"]), len(case["bases"])
    dev = torch.device("cuda", eng.device)
    off, bases, which = _dev(eng, case["off"]), _dev(eng, case["bases"]), _dev(eng, case["which"])
    cols = [torch.full(s, 77, dtype=t, device=dev) for s, t in (((N, 4, 4), torch.int32), ((N,), torch.int32), ((N,), torch.float32), ((N,), torch.uint8))]
    ptrs = [c.data_ptr() for c in cols]
    motifs = [m.encode() for st in case["structures"] for m in st]
    data = np.frombuffer(b"".join(motifs), np.uint8).copy()
    moff = np.concatenate([[0], np.cumsum([len(m) for m in motifs])]).astype(np.int64)
    soff = np.concatenate([[0], np.cumsum([len(st) for st in case["structures"]])]).astype(np.int32)
    K = len(case["structures"])

    def call(off=off, bases=bases, which=which, cap=N, scores=(1, 1, 1), n_structs=K, n_bases=T, dst_ptrs=ptrs, host=(data, moff, soff)):
        dst = mtr_amd.CWindowStructureDst(*dst_ptrs, cap)
        st = eng.lib.mtr_window_structure_device(eng.h, host[0].ctypes.data, host[1].ctypes.data, host[2].ctypes.data, n_structs, off.data_ptr(), bases.data_ptr(),
                                                 which.data_ptr(), N, n_bases, *scores, None, C.byref(dst))
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
    for kw, status, words in ((dict(scores=(6, 1, 1)), "MTR_ERR_BAD_ARG", "gain = 6"), (dict(scores=(1, 0, 1)), "MTR_ERR_BAD_ARG", "mismatch = 0"),
                              (dict(scores=(1, 1, 4)), "MTR_ERR_BAD_ARG", "indel = 4"), (dict(n_structs=0), "MTR_ERR_BAD_ARG", "n_structs = 0"),
                              (dict(host=(data, moff_down, soff)), "MTR_ERR_BAD_ARG", "motif_off decreases at motif 1"),
                              (dict(dst_ptrs=[ptrs[0], None, ptrs[2], ptrs[3]]), "MTR_ERR_BAD_ARG", "NULL"),
                              (dict(off=_dev(eng, bad_off)), "MTR_ERR_BAD_ARG", "win_off at window 5 does not ascend"),
                              (dict(n_bases=T - 1), "MTR_ERR_BAD_ARG", "does not ascend from 0 to n_bases"),
                              (dict(which=_dev(eng, bad_which)), "MTR_ERR_BAD_ARG", f"window 9: win_struct {K} outside 0..{K - 1}"),
                              (dict(bases=_dev(eng, bad_bases)), "MTR_ERR_BAD_ARG", "win_bases at 11: code 4 is above 3"),
                              (dict(off=torch.from_numpy(case["off"])), "MTR_ERR_BAD_ARG", "win_off is not device memory"),
                              (dict(cap=N - 1), "MTR_ERR_OVERFLOW", f"destination holds {N - 1} windows, {N} needed")):
        got = call(**kw)
        assert got[0] == status and words in got[1], (kw.keys(), got)
        assert all((c == 77).all() for c in cols), kw.keys()
    assert call()[0] == "MTR_OK"
    _assert_ws(cols, want, "after the refusals")


# ---- from reads to the structure of the called alleles --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (2, 3))
def test_from_reads_to_the_structure_of_each_allele_and_to_calls_by_segment(eng, seed):
    reads, loci = cc.truth_reads(seed), cc.truth_loci()
    eng.upload(reads)
    sg = eng.genotype_catalog(loci, 1)
    win = eng.genotype_windows(sg)
    calls = eng.call_alleles(sg, "bases")
    cons = eng.allele_consensus(sg, win, calls, band_extra=cc.TRUTH_EXTRA)
    alleles = torch.arange(2 * len(loci), dtype=torch.int32, device=cons.off.device) // 2
    rows = {(("CAG",), (1, 1, 1)): ((58, [[0, 60, 20, 59]]), (94, [[0, 96, 32, 95]])),
            (("CAG", "CAA", "CAG"), (1, 1, 1)): ((60, [[0, 30, 10, 30], [30, 33, 1, 3], [33, 60, 9, 27]]), (96, [[0, 75, 25, 75], [75, 78, 1, 3], [78, 96, 6, 18]])),
            (("CAG", "CAA", "CAG"), (2, 3, 2)): ((120, [[0, 30, 10, 30], [30, 33, 1, 3], [33, 60, 9, 27]]), (192, [[0, 75, 25, 75], [75, 78, 1, 3], [78, 96, 6, 18]]))}
    for (st, scores), want in rows.items():
        ws = eng.window_structure([list(st), "GAA"], cons.off, cons.bases, alleles, *scores)
        for a in (0, 1):
            assert ws.score[a].item() == want[a][0] and ws.seg[a, :len(st)].cpu().tolist() == want[a][1], (st, scores, a, ws.seg[a].cpu().tolist())
        assert not ws.seg[2:].any() and not ws.score[2:].any() and not ws.skipped.any()            # the uncalled locus' alleles are empty windows
    text = mtr_amd.format_window_structure([["CAG", "CAA", "CAG"]] * 2 + ["GAA"] * 2, ws, names=["a0", "a1", "b0", "b1"]).decode().splitlines()
    assert text[0] == "a0\t120\t1.0000\tCAG*10[0,30)30\tCAA*1[30,33)3\tCAG*9[33,60)27" and text[2] == "b0\t0\t0.0000\tGAA*0[0,0)0"
    # the single reads: equal to the reference, not to the truth (a noisy read's best structure need not be the true one)
    per_read = eng.window_structure([["CAG", "CAA", "CAG"], "GAA"], win.off, win.bases, sg.locus)
    off, bases = win.off.cpu().numpy(), win.bases.cpu().numpy()
    windows = [bases[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    _assert_ws(per_read, ref.columns([["CAG", "CAA", "CAG"], ["GAA"]], windows, sg.locus.cpu().tolist()), "per read")
    # all but one read of each allele hold the true count of the first segment, so the lower medians are the truth
    first = mtr_amd.with_segment_copies(sg, per_read, 0)
    assert torch.equal(first.fields[:, 3], per_read.seg[:, 0, 2]) and torch.equal(first.ratio, per_read.ratio)
    assert all(torch.equal(first.fields[:, k], sg.fields[:, k]) for k in (0, 1, 2, 4, 5, 6, 7)) and all(torch.equal(x, y) for x, y in zip(first[2:8] + first[9:10], sg[2:8] + sg[9:10]))
    by_segment = eng.call_alleles(first, "copies")
    assert by_segment.zygosity.cpu().tolist() == [2, 0] and by_segment.call[0].cpu().tolist() == [10, 25]
    last = eng.call_alleles(mtr_amd.with_segment_copies(sg, per_read, 2), "copies")
    assert last.zygosity.cpu().tolist() == [2, 0] and last.call[0].cpu().tolist() == [6, 9]
