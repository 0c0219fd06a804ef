"""The motif catalogue's truth for the tests, written from the definitions of include/mtr_hip.h alone: a brute force over all 2p rotations
of a unit and its reverse complement, the smallest divisor that is a period, and a dict aggregation into groups.  Nothing here calls the
product (mtr_amd.canonical_motif included).  start_slot() restates the grouping's internal hash (mtr_amd/csrc/unit_motif.h) so that a test
can build motifs that meet in the table; tests/test_unit_motif_host.py pins it to the header."""
import numpy as np

COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def rc(u: bytes) -> bytes:
    return u.translate(COMPLEMENT)[::-1]


def brute(u: bytes):
    """-> (motif, strand, rotation, motif_len)"""
    p = len(u)
    if p == 0:
        return b"", 0, 0, 0
    best, strand, rotation = None, 0, 0
    for st, s in enumerate((u, rc(u))):                       # the forward strand and the smaller rotation first: only a smaller string replaces
        d = s + s
        for r in range(p):
            c = d[r:r + p]
            if best is None or c < best:
                best, strand, rotation = c, st, r
    d = next(d for d in range(1, p + 1) if p % d == 0 and best[d:] + best[:d] == best)
    return best[:d], strand, rotation, d


def catalogue(units, read, copies, repeat_len):
    """the whole catalogue of rows (unit bytes, read, num_freq_unit, repeat_len) as a dict of lists / arrays named as ReportMotifs' columns"""
    per = [brute(u) for u in units]
    groups, order = {}, []
    for k, (motif, _, _, d) in enumerate(per):
        if motif not in groups:
            groups[motif] = dict(first=k, repeats=0, reads=set(), copies=0, bases=0)
            order.append(motif)
        g = groups[motif]
        g["repeats"] += 1
        g["reads"].add(int(read[k]))
        g["copies"] += int(copies[k]) * (len(units[k]) // d) if d else 0
        g["bases"] += int(repeat_len[k])
    index = {m: i for i, m in enumerate(order)}
    off = np.zeros(len(order) + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in order])
    return dict(strand=np.array([s for _, s, _, _ in per], np.uint8), rotation=np.array([r for _, _, r, _ in per], np.int32),
                motif_len=np.array([d for _, _, _, d in per], np.int32), group=np.array([index[m] for m, _, _, _ in per], np.int32),
                motif_off=off, motifs=np.frombuffer(b"".join(order), np.uint8),
                g_first=np.array([groups[m]["first"] for m in order], np.int32), g_repeats=np.array([groups[m]["repeats"] for m in order], np.int32),
                g_reads=np.array([len(groups[m]["reads"]) for m in order], np.int32), g_copies=np.array([groups[m]["copies"] for m in order], np.int64),
                g_bases=np.array([groups[m]["bases"] for m in order], np.int64))


def assert_catalogue(got, want, what=""):
    """got: a ReportMotifs of numpy arrays or tensors; want: catalogue()'s dict.  Every column, with its dtype."""
    for name, w in want.items():
        g = getattr(got, name)
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        assert g.dtype == w.dtype, (what, name, g.dtype, w.dtype)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: column {name} differs at {bad[:8].tolist()} ({len(bad)} of {len(w)}): got {g[bad[:8]].tolist()}, want {w[bad[:8]].tolist()}")


M64 = (1 << 64) - 1


def motif_hash(motif: bytes) -> int:
    """FNV-1a, 64 bits, over the motif's length (four bytes, low first) and its bytes"""
    h = 0xcbf29ce484222325
    for c in len(motif).to_bytes(4, "little") + motif:
        h = ((h ^ c) * 0x100000001b3) & M64
    return h


def start_slot(motif: bytes, slots: int) -> int:
    h = motif_hash(motif)
    return (h ^ (h >> 32)) & 0xffffffff & (slots - 1)


def random_units(rng, n, max_len=500):
    """n units of length 1..max_len, each a random root repeated p / d times (d a random divisor of p)"""
    out = []
    for _ in range(n):
        p = int(rng.randint(1, max_len + 1))
        divs = [d for d in range(1, p + 1) if p % d == 0]
        d = divs[int(rng.randint(0, len(divs)))]
        root = bytes(b"ACGT"[c] for c in rng.randint(0, 4, size=d))
        out.append(root * (p // d))
    return out


WORKED = [(b"GT", b"AC", 1, 0, 2), (b"ACAC", b"AC", 0, 0, 2), (b"AT", b"AT", 0, 0, 2), (b"ACGT", b"ACGT", 0, 0, 4),
          (b"TTTTA", b"AAAAT", 1, 1, 5), (b"CAG", b"AGC", 0, 1, 3), (b"CTG", b"AGC", 1, 1, 3)]
