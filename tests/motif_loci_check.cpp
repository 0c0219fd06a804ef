// motif_loci_check.cpp — the host's check of what the known-motif locus search adds to the per-lane code: a program of its own (the form a
// sanitizer build runs).
//   1. the WINDOWED lane DP (mtr_amd/csrc/motif_dp.h with a first base lo): aligning x[lo .. hi) inside the packed read gives, in all nine outputs,
//      what the unwindowed DP gives for the substring copied out and packed by itself - the coordinates are the window's own, the kernels raise
//      them by lo.  lo takes all 16 phases of a word, windows end on the read's last base (the packed read holds exactly the words it touches:
//      a load past them is the address sanitizer's), windows of one row, every bucket at its smallest and largest U, and 64 lanes of unequal
//      windows of ONE read set share one interleaved cell buffer, all forward passes before all tracebacks.
//   2. the split rule (mtr_amd/csrc/motif_loci.h, mlo_split) against the definition's three lines written out naively, over every hit position of
//      small windows: hits that touch lo or hi (empty children), children of exactly minlen - 1 and minlen bases, the last depth (open).
//   3. the length classes: monotone, inside MLO_N_CLASSES up to the lane path's longest window, a class no wider than a sixteenth of its lengths.
#include "../mtr_amd/csrc/motif_dp.h"
#include "../mtr_amd/csrc/motif_loci.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

static std::vector<uint32_t> pack(const std::vector<uint8_t> &x)
{
    std::vector<uint32_t> w((x.size() + 15) / 16, 0u);
    for (size_t i = 0; i < x.size(); i++) w[i >> 4] |= (uint32_t)(x[i] & 3) << (30 - 2 * (i & 15));
    return w;
}

static uint32_t g_x = 88172645u;
static uint32_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5; return g_x; }

// a read with tandem stretches of m between random bases, so that windows cut hits in every way
static std::vector<uint8_t> make_read(int L, const std::vector<uint8_t> &m)
{
    std::vector<uint8_t> x((size_t)L);
    const int U = (int)m.size();
    int i = 0;
    while (i < L) {
        const int run = 1 + (int)(rnd() % 40);
        const bool tandem = (rnd() & 1) != 0;
        int ph = (int)(rnd() % (uint32_t)U);
        for (int k = 0; k < run && i < L; k++, i++) {
            if (tandem && rnd() % 13 != 0) { x[(size_t)i] = m[(size_t)(ph % U)]; ph++; }
            else x[(size_t)i] = (uint8_t)(rnd() & 3);
        }
    }
    return x;
}

template <int UB>
static MotifHit run_bucket(const uint32_t *pk, int L, uint64_t mot, int U, int G, int MM, int D, const MdpCellsLane &c, bool forward_only, int *best, int lo)
{
    if (forward_only) { motif_dp_forward<UB>(pk, L, mot, U, G, MM, D, c, best[0], best[1], best[2], lo); return MotifHit{}; }
    return motif_dp_traceback(c, U, best[0], best[1], best[2]);
}
static MotifHit run(const uint32_t *pk, int L, uint64_t mot, int U, int G, int MM, int D, const MdpCellsLane &c, bool forward_only, int *best, int lo)
{
    switch (mdp_bucket(U)) {
    case 4: return run_bucket<4>(pk, L, mot, U, G, MM, D, c, forward_only, best, lo);
    case 8: return run_bucket<8>(pk, L, mot, U, G, MM, D, c, forward_only, best, lo);
    case 16: return run_bucket<16>(pk, L, mot, U, G, MM, D, c, forward_only, best, lo);
    default: return run_bucket<32>(pk, L, mot, U, G, MM, D, c, forward_only, best, lo);
    }
}
// the unwindowed DP of a sequence by itself (one lane, a buffer of its own)
static MotifHit alone(const std::vector<uint8_t> &x, const std::vector<uint8_t> &m, int G, int MM, int D)
{
    const int U = (int)m.size(), nd = mdp_dwords(U);
    std::vector<uint32_t> cells(std::max<size_t>(x.size(), 1) * (size_t)nd * 64, 0xeeeeeeeeu);
    const std::vector<uint32_t> pk = pack(x);
    const MdpCellsLane c = { cells.data(), nd, 17 };
    int best[3];
    (void)run(pk.data(), (int)x.size(), mdp_motif_bits(m.data(), U), U, G, MM, D, c, true, best, 0);
    return run(nullptr, 0, 0, U, G, MM, D, c, false, best, 0);
}

static long g_checked = 0, g_hits = 0;

struct Win { int lo, hi; };
// 64 lanes, lane l with window w[l] of the one read x (lo == hi: a lane without a task), one buffer of the size the host gives a wavefront
static bool check_group(const std::vector<uint8_t> &x, const std::vector<Win> &w, const std::vector<uint8_t> &m, int G, int MM, int D)
{
    const int U = (int)m.size(), nd = mdp_dwords(U);
    size_t rows = 0;
    for (const Win &v : w) rows = std::max(rows, (size_t)(v.hi - v.lo));
    std::vector<uint32_t> cells(std::max<size_t>(rows, 1) * (size_t)nd * 64, 0xeeeeeeeeu);
    const uint64_t mot = mdp_motif_bits(m.data(), U);
    const std::vector<uint32_t> pk = pack(x);
    int best[64][3];
    for (int l = 0; l < 64; l++) {
        const MdpCellsLane c = { cells.data(), nd, l };
        (void)run(pk.data(), w[(size_t)l].hi - w[(size_t)l].lo, mot, U, G, MM, D, c, true, best[l], w[(size_t)l].lo);
    }
    bool ok = true;
    for (int l = 0; l < 64; l++) {
        const Win v = w[(size_t)l];
        if (v.hi == v.lo) continue;
        const MdpCellsLane c = { cells.data(), nd, l };
        const MotifHit got = run(nullptr, 0, mot, U, G, MM, D, c, false, best[l], 0);
        const MotifHit want = alone(std::vector<uint8_t>(x.begin() + v.lo, x.begin() + v.hi), m, G, MM, D);
        g_checked++; g_hits += want.score > 0;
        if (memcmp(&got, &want, sizeof got) != 0) {
            fprintf(stderr, "U %d window %d..%d of %zu scores %d %d %d lane %d: got (%d %d %d %d %d %d %d %d %d), want (%d %d %d %d %d %d %d %d %d)\n", U, v.lo, v.hi, x.size(),
                    G, MM, D, l, got.start, got.end, got.repeat_len, got.copies, got.mat, got.mis, got.ins, got.del, got.score,
                    want.start, want.end, want.repeat_len, want.copies, want.mat, want.mis, want.ins, want.del, want.score);
            ok = false;
        }
    }
    return ok;
}

static bool check_windows()
{
    static const int scores[4][3] = { { 5, 1, 1 }, { 1, 1, 3 }, { 1, 3, 1 }, { 1, 1, 1 } };
    bool ok = true;
    for (int U : { 1, 4, 5, 8, 9, 16, 17, 32 }) {                    // every bucket's smallest and largest U
        std::vector<uint8_t> m((size_t)U);
        for (auto &c : m) c = (uint8_t)(rnd() % (U > 2 ? 3u : 4u));
        for (const auto &s : scores) {
            for (int L : { 37, 64, 131 }) {                              // reads that end inside a word, on a word, and after several
                const std::vector<uint8_t> x = make_read(L, m);
                std::vector<Win> w(64, Win{ 0, 0 });
                // every phase of lo with the window ending on the read's last base; then the same phases with one row
                for (int l = 0; l < 16; l++) w[(size_t)l] = { std::min(l, L - 1), L };
                for (int l = 16; l < 32; l++) w[(size_t)l] = { std::min(l + 1, L - 1), std::min(l + 1, L - 1) + 1 };
                w[32] = { L - 1, L };                                    // the last base alone
                w[33] = { 0, L };                                        // the whole read: the unwindowed call
                for (int l = 34; l < 64; l++) {                          // unequal windows anywhere; some lanes without a task
                    if (l % 9 == 4) continue;
                    const int lo = (int)(rnd() % (uint32_t)L), len = 1 + (int)(rnd() % (uint32_t)(L - lo));
                    w[(size_t)l] = { lo, lo + len };
                }
                ok = check_group(x, w, m, s[0], s[1], s[2]) && ok;
            }
        }
    }
    return ok;
}

// ---- the split rule ---------------------------------------------------------------------------------------------------------------------
static long g_splits = 0, g_edges = 0;
static bool check_split()
{
    bool ok = true;
    for (int R : { 1, 2, 5 })
        for (int minlen : { 1, 2, 3, 7 })
            for (int lo : { 0, 5 })
                for (int len = 1; len <= 24; len++)
                    for (int depth = 0; depth < R; depth++)
                        for (int start = 0; start < len; start++)
                            for (int end = start; end < len; end++)
                                for (int score : { 0, 3, 4, 9 }) {
                                    const int S = 4, hi = lo + len;
                                    const MloSplit got = mlo_split(lo, hi, depth, R, minlen, S, score, start, end);
                                    // the definition: loci(lo, lo + start, depth + 1) and loci(lo + end + 1, hi, depth + 1), each of which returns at once if
                                    // it is shorter than minlen, and sets open if depth + 1 == R
                                    int emit = score >= S, n = 0, open = 0, clo[2] = { 0, 0 }, chi[2] = { 0, 0 };
                                    if (emit) {
                                        const int a[2] = { lo, lo + end + 1 }, b[2] = { lo + start, hi };
                                        for (int k = 0; k < 2; k++) {
                                            if (b[k] - a[k] < minlen) continue;
                                            if (depth + 1 == R) open = 1; else { clo[n] = a[k]; chi[n] = b[k]; n++; }
                                        }
                                    }
                                    g_splits++;
                                    g_edges += emit && (start == 0 || end == len - 1 || start == minlen || start == minlen - 1);
                                    bool same = got.emit == emit && got.n == n && got.open == open;
                                    for (int k = 0; same && k < n; k++) same = got.clo[k] == clo[k] && got.chi[k] == chi[k];
                                    for (int k = 0; same && k < got.n; k++) same = got.chi[k] - got.clo[k] >= minlen && got.clo[k] >= lo && got.chi[k] <= hi && got.chi[k] - got.clo[k] < len;
                                    if (!same) { fprintf(stderr, "split: window %d..%d depth %d of %d minlen %d score %d hit %d..%d\n", lo, hi, depth, R, minlen, score, start, end); ok = false; }
                                }
    for (int G = 1; G <= 5; G++)
        for (int S = 1; S <= 40; S++) {
            const int ml = mlo_minlen(S, G);
            if (!(ml * G >= S && (ml - 1) * G < S)) { fprintf(stderr, "minlen(%d, %d) = %d\n", S, G, ml); ok = false; }
        }
    return ok;
}

static bool check_classes()
{
    bool ok = true;
    int prev = 0, first_of = 1;                       // (class 0 is no window's: len >= 1)
    for (int len = 1; len <= 16384; len++) {
        const int c = mlo_len_class(len);
        if (c < prev || c > prev + 1 || c < 0 || c >= MLO_N_CLASSES) { fprintf(stderr, "class(%d) = %d after %d\n", len, c, prev); ok = false; }
        if (c != prev) first_of = len;
        if ((len - first_of) * 16 > first_of) { fprintf(stderr, "class %d holds %d .. %d\n", c, first_of, len); ok = false; }
        prev = c;
    }
    return ok && prev == MLO_N_CLASSES - 1;
}

int main()
{
    const bool w = check_windows(), s = check_split(), c = check_classes(), ok = w && s && c;
    printf("%ld windows checked (%ld with a hit), %ld splits (%ld at an edge): %s\n", g_checked, g_hits, g_splits, g_edges, ok ? "ok" : "FAILED");
    return ok && g_hits > g_checked / 4 && g_edges > 1000 ? 0 : 1;
}
