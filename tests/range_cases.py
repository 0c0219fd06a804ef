"""The seeded reads on which the three-kernel range finder (launch_k1_parts, mtr_amd/csrc/mtr_abi.hip) is held to the oracle's ranges
(tests/test_gpu_ranges_parts.py), and the arithmetic of that path that decides which reads they are.

Every length below is read from the code; tests/test_range_cases_ref.py asserts with the CPU oracle that each read is what its claim says,
so a later change of a constant makes the case list fail instead of quietly no longer covering the path.

  passes      a pass (k, w) exists when w < L // 2: L = 2w + 1 / 2w + 2 for every window, and L = 1, 2, 10 with no pass at all (no work item:
              mtr_k1_part(K1_PASSES) is not launched).  L >= 2 562: 17 passes, pass 16 is wavefront 0's second turn in the extraction
              pipeline (K1_PIPE_WAVES = 16).  L >= 20 482: all 20.
  segments    n = L + 2 rand_len(L) positions, cut into segments of max(512, roundup64(ceil(n / 64))): n = 512 / 513, 1 024 / 1 025,
              L = 999 / 1 000 / 1 010 (rand_len changes from 100 to L // 10), n = 32 768 / 32 769 (the segment grows from 512 to 576).
  phase D     the compact list of the alive entries lives in LDS while (cnt + 1) * 20 fits the pipeline's 128 KB arena (cnt <= 6 552);
              beyond, the chain runs on the global lists (k1_dedup_range), through the 6 144-entry LDS window (k1_dedup_window) where no
              wavefront but the first finds a cut in its slice of the list.
"""
from __future__ import annotations

import numpy as np

MIN_WINDOW, MAX_WINDOW = 5, 10240                 # MTRC_MIN_WINDOW, MTRC_MAX_WINDOW
WINDOWS = [MIN_WINDOW << t for t in range(12)]    # 5 .. 10 240
ALL_PASSES = [(1, w) for w in WINDOWS if w <= 20] + [(3, w) for w in WINDOWS if w <= 80] + [(5, w) for w in WINDOWS]      # pass index -> (k, w)
PARTS_MAX = 256                                   # launch_staged: parts_max
PIPE_WAVES, TILE = 16, 512                        # K1_PIPE_WAVES, K1_TILE
LIST_ARENA_BYTES = PIPE_WAVES * TILE * 16         # K1_PIPE_ARENA_BYTES
LDS_LIST_MAX = LIST_ARENA_BYTES // 20 - 1         # the largest cnt with (cnt + 1) * 20 <= arena: 6 552
DEDUP_WINDOW = 6144                               # K1_WIN


def rand_len(L):
    return 100 if L < 1000 else L // 10            # mtrc_rand_len


def padded_len(L):
    return L + 2 * rand_len(L)


def seg_len(n):
    return max(512, (((n + 63) // 64) + 63) // 64 * 64)      # k1_seg_len


def n_segments(L):
    n = padded_len(L)
    return (n + seg_len(n) - 1) // seg_len(n)


def passes(L):
    """the (k, w) passes of a read of L bases, in the order the kernels enumerate them"""
    return [(k, w) for k, w in ALL_PASSES if w < L // 2]


def work_items(L):
    return len(passes(L)) * n_segments(L)


def no_cut(raw):
    """raw: the oracle's list before the de-duplication, rows (start, end, w, k).  True where k1_lists_wg hands the whole chain to
    one wavefront: none of the wavefronts 1 .. 15 finds, in its slice of the list, an entry that starts beyond every earlier end."""
    cnt = len(raw)
    sper = ((cnt + PIPE_WAVES - 1) // PIPE_WAVES + 63) // 64 * 64
    if cnt <= sper:
        return True
    before = np.maximum.accumulate(raw[:, 1])[:-1]            # before[i - 1]: the largest end in front of entry i
    return bool(np.all(raw[sper:, 0] <= before[sper - 1:]))


# ---- content ---------------------------------------------------------------------------------------------------------------------------
def random_read(rng, L):
    return rng.randint(0, 4, size=L).astype(np.uint8)


def noisy_repeat(rng, L, unit_len, err):
    """L bases of a tandem repeat of a random unit, every base hit with probability err by a substitution, an insertion or a deletion"""
    unit = rng.randint(0, 4, size=unit_len)
    src = np.tile(unit, (L + L // 2) // unit_len + 2)
    out, i = [], 0
    hit = rng.random_sample(len(src)) < err
    kind = rng.randint(0, 3, size=len(src))
    sub = rng.randint(1, 4, size=len(src))
    ins = rng.randint(0, 4, size=len(src))
    while len(out) < L:
        b = int(src[i])
        if hit[i]:
            if kind[i] == 0:
                out.append((b + int(sub[i])) & 3)
            elif kind[i] == 1:
                out.append(int(ins[i])); out.append(b)
        else:
            out.append(b)
        i += 1
    return np.array(out[:L], np.uint8)


def mostly_repeats(rng, L):
    """noisy tandem repeats of units of 1, 3, 7, 20 and 50 bases at 3 % .. 20 % errors, short random stretches between them"""
    parts, have = [], 0
    while have < L:
        u = (1, 3, 7, 20, 50)[rng.randint(0, 5)]
        lo = max(12, 4 * u)
        span = int(rng.randint(lo, max(lo, min(L, 40 * u + L // 4)) + 1))
        parts.append(noisy_repeat(rng, span, u, rng.uniform(0.03, 0.20)))
        parts.append(random_read(rng, int(rng.randint(0, 40))))
        have += len(parts[-1]) + len(parts[-2])
    return np.concatenate(parts)[:L].astype(np.uint8)


def with_clean_repeat(rng, L, start, length, unit_len):
    c = random_read(rng, L)
    c[start:start + length] = np.tile(rng.randint(0, 4, size=unit_len), length // unit_len + 1)[:length]
    return c


# ---- the reads ------------------------------------------------------------------------------------------------------------------------
class Case:
    """lists: what phase D does with the read in BOTH DI modes - "lds" (cnt < 6 000), "cuts" (cnt > 7 000, a later wavefront finds a cut: k1_dedup_range
    on the global lists), "window" (cnt > 7 000 and no cut: k1_dedup_window)"""

    def __init__(self, name, codes, lists="lds"):
        self.name, self.codes, self.lists = name, np.ascontiguousarray(codes, np.uint8), lists
        self.L = len(self.codes)


def _seeded(tag, L):
    return np.random.RandomState((sum(ord(ch) * (i + 1) for i, ch in enumerate(tag)) * 7919 + L) % (2 ** 31))


_CASES = None


def cases():
    """name -> Case; built once, never modified"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    # pass thresholds: the pass of window w is absent at 2w + 1, present at 2w + 2; none at all at 1, 2, 10
    for L in (1, 2, 10):
        out.append(Case(f"nopass_{L}", random_read(_seeded("nopass", L), L)))
    for t, w in enumerate(WINDOWS):
        for L in (2 * w + 1, 2 * w + 2):
            rng = _seeded("threshold", L)
            out.append(Case(f"threshold_{L}", mostly_repeats(rng, L) if t % 2 == 0 else random_read(rng, L)))
    # segment edges: n = 512 / 513, 1 024 / 1 025, rand_len's step at 1 000, n = 32 768 / 32 769 (segments of 512 / 576)
    for L in (312, 313, 824, 825, 999, 1000, 1010, 27308, 27309):
        rng = _seeded("segment", L)
        out.append(Case(f"segment_{L}", mostly_repeats(rng, L) if L % 2 == 0 else random_read(rng, L)))
    # content
    out.append(Case("random_2000", random_read(_seeded("random", 2000), 2000)))
    out.append(Case("random_5003", random_read(_seeded("random", 5003), 5003)))
    for u, err, L in ((1, 0.03, 2563), (3, 0.10, 3001), (7, 0.20, 4100), (20, 0.05, 5500), (50, 0.15, 6007)):
        rng = _seeded(f"unit{u}", L)
        c = np.concatenate([random_read(rng, 150), noisy_repeat(rng, L - 300, u, err), random_read(rng, 150)])
        out.append(Case(f"repeat_u{u}_{L}", c))
    # a clean repeat across segment and tile boundaries: padded positions 900 .. 2 300 of segments of 512 (read position + 600), and
    # padded positions 3 300 .. 5 100 of segments of 576 (read position + 3 000)
    out.append(Case("clean_6000", with_clean_repeat(_seeded("clean", 6000), 6000, 300, 1400, 7)))
    out.append(Case("clean_30000", with_clean_repeat(_seeded("clean", 30000), 30000, 300, 1800, 20)))
    # phase D beyond the LDS lists
    # (seeds chosen so that the claim holds in both DI modes; tests/test_range_cases_ref.py asserts it)
    out.append(Case("big_cuts_60000", noisy_repeat(np.random.RandomState(6), 60000, 7, 0.20), lists="cuts"))
    out.append(Case("big_window_60000", noisy_repeat(np.random.RandomState(5), 60000, 50, 0.15), lists="window"))
    out.append(Case("big_window_u7_60000", noisy_repeat(np.random.RandomState(2), 60000, 7, 0.20), lists="window"))
    _CASES = {c.name: c for c in out}
    assert len(_CASES) == len(out)
    return _CASES


_MIXED = ["threshold_12", "threshold_20482", "big_cuts_60000", "nopass_2", "repeat_u7_4100", "big_window_60000", "segment_27309", "threshold_2562", "nopass_10",
          "big_window_u7_60000", "threshold_11"]


def batches():
    """name -> list of case names; every batch is at most PARTS_MAX reads.  "mixed" puts L = 12 next to 20 482 and 60 000 (the scratch slice and
    the layout are sized by the longest read of the batch, not by the read's own length), "single" is one read of it, "mixed_reversed" its reverse."""
    names = list(cases())
    rest = [n for n in names if not n.startswith("big_")]
    return {"thresholds_and_segments": [n for n in rest if n.startswith(("nopass", "threshold", "segment"))],
            "content": [n for n in rest if not n.startswith(("nopass", "threshold", "segment"))],
            "mixed": list(_MIXED), "single": ["threshold_20482"], "mixed_reversed": list(reversed(_MIXED))}
