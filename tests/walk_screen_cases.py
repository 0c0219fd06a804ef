"""Crafted reads and ranges for the dead-range screen of the staged unit search (mtr_amd/csrc/walk_screen.h), shared by its CPU test
(tests/test_walk_screen_host.py) and its GPU test (tests/test_gpu_walk_screen.py).  A range is (qs, qe, w): the window and the width class
that decides its k range (w < 100: k = 2..10, w < 1000: k = 2..12, else k = 5..15)."""
import numpy as np

A, C_, G, T = 0, 1, 2, 3


def pack(codes: np.ndarray) -> np.ndarray:
    """2 bits per base, first base in the top bits of word 0 (BatchView::packed), three zero words behind the read"""
    L = len(codes)
    padded = np.zeros((L + 15) // 16 * 16, np.uint32)
    padded[:L] = codes
    shifts = (30 - 2 * (np.arange(16, dtype=np.uint32))).astype(np.uint32)
    words = np.bitwise_or.reduce(padded.reshape(-1, 16) << shifts, axis=1).astype(np.uint32)
    return np.concatenate([words, np.zeros(3, np.uint32)])


def _rand(rng, n, first_not=None, last_not=None):
    r = rng.randint(0, 4, size=n).astype(np.uint8)
    if n and first_not is not None and r[0] == first_not:
        r[0] = (first_not + 1) % 4
    if n and last_not is not None and r[-1] == last_not:
        r[-1] = (last_not + 1) % 4
    return r


def crafted():
    """-> list of (name, codes, ranges)"""
    rng = np.random.RandomState(64)
    out = []

    def embedded(name, core, widths=(5, 160)):
        core = np.asarray(core, np.uint8)
        pre, post = _rand(rng, 50, last_not=int(core[0])), _rand(rng, 50, first_not=int(core[-1]))
        codes = np.concatenate([pre, core, post])
        s, e = 50, 50 + len(core) - 1
        rs = []
        for w in widths:
            rs += [(s, e, w), (s - 1, e, w), (s, e + 1, w), (s - 3, e + 4, w), (s + 1, e - 1, w)]
        out.append((name, codes, rs))

    embedded("ac_x5", [A, C_] * 5)
    embedded("ac_x6", [A, C_] * 6)
    embedded("a_x6", [A] * 6)
    embedded("a_x7", [A] * 7)
    embedded("t_x6", [T] * 6)                      # (a trailing raw T aliases the 2-mer AT, not TT)
    embedded("acg_x22", [A, C_, G] * 22)           # 66 bases: windows of 64 (the rule's widest) and 65 (excluded) inside
    out[-1][2].extend([(50, 113, 5), (50, 114, 5), (51, 114, 160), (50, 114, 160), (40, 103, 5), (40, 104, 5)])
    plain = rng.randint(0, 4, size=120).astype(np.uint8)
    out.append(("windows_of_5_and_6", plain, [(10, 14, 5), (10, 15, 5), (31, 35, 160), (31, 36, 160), (60, 64, 5), (61, 66, 5)]))
    # ranges at the read's end, where the window's trailing raw nodes count (every k with qe > L - k + 1 has more than one)
    for L in (30, 31, 47, 64, 100, 200):
        for tail in ([A, G] * 8, [A] * 9, [C_, A, T, G, G, T, A, C_, C_, G]):
            body = _rand(rng, L - len(tail), last_not=tail[0])
            codes = np.concatenate([body, np.asarray(tail, np.uint8)])
            rs = []
            for back in range(0, 11):              # back = 0: the last base, 1: the last two bases are behind / at the window's end, ...
                qe = L - 1 - back
                for width in (5, 6, 12, 17):
                    if qe - width + 1 >= 0:
                        rs += [(qe - width + 1, qe, 5), (qe - width + 1, qe, 160)]
            out.append((f"end_L{L}_{len(out)}", codes, rs))
    out.append(("w_1280_over_a_short_window", plain, [(10, 30, 1280), (10, 30, 1000), (10, 30, 640)]))
    return out


def long_reads():
    """two reads of at least 2 600 bases whose widest window has w >= 1 280 (the range finder takes that window from ~5 kb of repeat on)"""
    from mtr_amd import synth
    rng = np.random.RandomState(1280)
    return [synth.make_read(rng, u, copies, pre, post)[0] for u, copies, pre, post in ((200, 25, 50, 50), (150, 36, 100, 60))]
