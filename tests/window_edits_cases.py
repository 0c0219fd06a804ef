"""The inputs of the window-edits tests (CPU and GPU): those of tests/window_structure_cases.py - every column bucket at its edges with both
counter widths, window starts at every residue of 16, more structures than a wavefront has lanes, window counts either side of a wavefront - and
every window length from 0 to 33 (a stored row is whole 32-bit words of its own, so the rows have no packing boundary; the lengths run over every
boundary of the window's 8-byte loads and of the rows a wavefront's slot is sized by).  The reference's answers are computed once per process
and shared."""
import numpy as np

from tests import window_edits_ref as ref
from tests import window_structure_cases as wc

LENGTHS = tuple(range(34))
SCORES = wc.SCORES
COUNTS = wc.COUNTS


def lengths_case():
    """n = 0 .. 33 for one structure of every bin: <8, narrow>, <16, narrow>, <32, narrow>, <8, wide>, <16, wide>"""
    rng = np.random.default_rng(11)
    structures = [["CAG"], ["CAGCAGG", "CCGTT"], ["ACGTTGCAAGCTTAGGCAT", "CCG"], ["CA", "G", "TC", "AAG"], ["CAG", "CAACAG", "CCGCCA", "T"]]
    windows, which = [], []
    for k, st in enumerate(structures):
        for n in LENGTHS:
            windows.append(wc.window_of(rng, st, n, 0.15))
            which.append(k)
    return wc.case(structures, windows, which)


def all_cases():
    out = wc.all_cases()
    out["lengths"] = lengths_case()
    return out


_cache = {}


def expected():
    """{(name, scores): (case, the reference's five columns)}, computed once per process and shared by the tests; nobody changes it"""
    if not _cache:
        for name, c in all_cases().items():
            for sc in SCORES:
                _cache[(name, sc)] = (c, ref.columns(c["structures"], c["windows"], c["which"], *sc))
    return _cache
