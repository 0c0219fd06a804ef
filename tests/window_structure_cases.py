"""The inputs of the window-structure tests (CPU and GPU): structures and windows chosen where the kernels can go wrong - every column bucket at
its edges with both counter widths, window lengths either side of the 8-byte load, window starts at every residue of 16, more structures than a
wavefront has lanes, window counts either side of a wavefront - and the reference's answers, computed once per process and shared."""
import numpy as np

from tests import window_structure_ref as ref

LETTERS = "ACGT"
WIDTHS_NARROW = (1, 7, 8, 9, 15, 16, 17, 31, 32)          # S <= 2
WIDTHS_WIDE = (8, 9, 16)                                  # S = 3 and 4
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 33)
COUNTS = (0, 1, 63, 64, 65, 257)
SCORES = ((1, 1, 1), (2, 3, 2))
HAND = [   # (window, structure, scores, score, the used segments' (start, end, copies, matches)): worked out by hand from the definition
    ("CAG" * 10 + "CAA" + "CAG" * 9, ["CAG"], (1, 1, 1), 58, [(0, 60, 20, 59)]),
    ("CAG" * 10 + "CAA" + "CAG" * 9, ["CAG", "CAA", "CAG"], (1, 1, 1), 60, [(0, 30, 10, 30), (30, 33, 1, 3), (33, 60, 9, 27)]),
    ("CAG" * 10 + "CAA" + "CAG" * 9, ["CAG", "CAA", "CAG"], (2, 3, 2), 120, [(0, 30, 10, 30), (30, 33, 1, 3), (33, 60, 9, 27)]),
    ("CAG" * 25 + "CAA" + "CAG" * 6, ["CAG"], (1, 1, 1), 94, [(0, 96, 32, 95)]),
    ("CAG" * 25 + "CAA" + "CAG" * 6, ["CAG", "CAA", "CAG"], (1, 1, 1), 96, [(0, 75, 25, 75), (75, 78, 1, 3), (78, 96, 6, 18)]),
    ("CAG" * 25 + "CAA" + "CAG" * 6, ["CAG", "CAA", "CAG"], (2, 3, 2), 192, [(0, 75, 25, 75), (75, 78, 1, 3), (78, 96, 6, 18)]),
    ("CAGCAGAGCAG", ["CAG"], (1, 1, 1), 10, [(0, 11, 4, 11)]),
    ("CAG" * 5 + "C" + "CCG" * 3, ["CAG", "CCG"], (1, 1, 1), 23, [(0, 16, 5, 15), (16, 25, 3, 9)]),
    ("TT", ["CAG", "CCG"], (1, 1, 1), -2, [(2, 2, 0, 0), (2, 2, 0, 0)]),
    ("", ["CAG"], (1, 1, 1), 0, [(0, 0, 0, 0)]),
]


def motif(rng, n, alphabet=4):
    return "".join(LETTERS[int(c)] for c in rng.integers(0, alphabet, n))


def structure_of(rng, S, W, alphabet=4):
    """S motifs of W bases in all, each of at least one"""
    cuts = sorted(rng.choice(np.arange(1, W), S - 1, replace=False).tolist()) if S > 1 else []
    return [motif(rng, b - a, alphabet) for a, b in zip([0] + cuts, cuts + [W])]


def window_of(rng, st, n, rate=0.1):
    """copies of the structure's motifs in order with errors, cut or padded to n bases"""
    y = []
    for m in st:
        for _ in range(int(rng.integers(0, 2 + n // (len(m) * len(st))))):
            for c in m:
                e = rng.random()
                if e < rate / 3:
                    y.append(int(rng.integers(0, 4)))
                elif e < 2 * rate / 3:
                    y += [LETTERS.index(c), int(rng.integers(0, 4))]
                elif e >= rate:
                    y.append(LETTERS.index(c))
    y += rng.integers(0, 4, max(0, n - len(y))).tolist()
    return np.array(y[:n], np.uint8)


def case(structures, windows, which):
    off = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int64)
    bases = np.concatenate([np.asarray(w, np.uint8) for w in windows] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    return dict(structures=structures, windows=windows, off=off, bases=bases, which=np.asarray(which, np.int32))


def widths_case():
    """every width at the buckets' edges x every length either side of the load, S = 1 and 2 narrow, 3 and 4 wide"""
    rng = np.random.default_rng(7)
    structures = [structure_of(rng, S, W, 3) for W in WIDTHS_NARROW for S in (1, 2) if S <= W] + [structure_of(rng, S, W, 3) for W in WIDTHS_WIDE for S in (3, 4)]
    windows, which = [], []
    for k, st in enumerate(structures):
        for n in LENGTHS:
            windows.append(window_of(rng, st, n))
            which.append(k)
    return case(structures, windows, which)


def residues_case():
    """16 windows of 17 bases and 16 of 33: the starts run through every residue of 16"""
    rng = np.random.default_rng(8)
    structures = [["CAG"], ["CAG", "CCG"], ["AC", "G", "T", "CAGG"]]
    which = [k % 3 for k in range(32)]
    windows = [window_of(rng, structures[which[k]], 17 if k < 16 else 33) for k in range(32)]
    return case(structures, windows, which)


def lanes_case():
    """130 windows of 130 different structures: two wavefronts and a bit, no two lanes of one alike"""
    rng = np.random.default_rng(9)
    structures = []
    while len(structures) < 130:
        st = structure_of(rng, int(rng.integers(1, 3)), int(rng.integers(3, 9)))
        if st not in structures:
            structures.append(st)
    windows = [window_of(rng, st, int(rng.integers(20, 41))) for st in structures]
    return case(structures, windows, list(range(130)))


def count_case(N):
    rng = np.random.default_rng(100 + N)
    structures = [["CAG"], ["CAGG", "CAGA", "CA"], ["A"], ["CAG", "CAACAG", "CCG", "T"]]
    which = [int(k) for k in rng.integers(0, 4, N)]
    windows = [window_of(rng, structures[k], int(rng.integers(0, 30))) for k in which]
    return case(structures, windows, which)


def all_cases():
    out = dict(widths=widths_case(), residues=residues_case(), lanes=lanes_case())
    out.update({f"count{N}": count_case(N) for N in COUNTS})
    return out


_cache = {}


def expected():
    """{(name, scores): (case, the reference's four columns)}, computed once per process and shared by the tests; nobody changes it"""
    if not _cache:
        for name, c in all_cases().items():
            for sc in SCORES:
                _cache[(name, sc)] = (c, ref.columns(c["structures"], c["windows"], c["which"], *sc))
    return _cache
