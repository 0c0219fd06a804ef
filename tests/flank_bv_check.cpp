// flank_bv_check.cpp — the per-lane scan of the flank search (mtr_amd/csrc/flank_bv.h) for the host: a program of its own (the form a sanitizer
// build runs) that compares dist, end and start of fbv_search<W>() with full-matrix DPs written here from the definition of include/mtr_hip.h.
// Both words; patterns of 1, 2, 31, 32, 33, 63 and 64 bases (the 32-bit word up to 32); texts of 0 and 1 bases, texts shorter than the pattern,
// texts of 15 / 16 / 17 and 31 / 32 / 33 bases (the packed words' edges), a hit planted on the text's first and on its last base, two planted
// hits of equal distance (the smaller end must win), windows that begin inside a word, and random texts with 0..4 edits in the planted copy.
// The packed text holds exactly the words the window touches, so a scan that loads beyond them trips the address sanitizer.  start is the
// largest s over ALL s <= end (the anchored full matrix gives ed(p, x[s .. end)) for every s); every eighth case computes each ed(p, x[s .. end))
// by a DP of its own as well.
#include "../mtr_amd/csrc/flank_bv.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef std::vector<uint8_t> Seq;

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }      // lo .. hi
static Seq rnd_seq(int n) { Seq s((size_t)n); for (auto &v : s) v = (uint8_t)(rnd() & 3u); return s; }

// ed(a, b): the whole matrix
static int ed(const Seq &a, const uint8_t *b, int nb)
{
    const int na = (int)a.size();
    std::vector<int> prev((size_t)nb + 1), cur((size_t)nb + 1);
    for (int j = 0; j <= nb; j++) prev[(size_t)j] = j;
    for (int i = 1; i <= na; i++) {
        cur[0] = i;
        for (int j = 1; j <= nb; j++)
            cur[(size_t)j] = std::min(prev[(size_t)j - 1] + (a[(size_t)i - 1] != b[j - 1] ? 1 : 0), std::min(prev[(size_t)j] + 1, cur[(size_t)j - 1] + 1));
        prev.swap(cur);
    }
    return prev[(size_t)nb];
}

// the definition on x[0 .. L)
static FbvHit naive(const Seq &p, const Seq &x, bool each_s)
{
    const int m = (int)p.size(), L = (int)x.size(), nr = m + 1;
    std::vector<int> D((size_t)(L + 1) * (size_t)nr);
    for (int i = 0; i <= m; i++) D[(size_t)i] = i;
    FbvHit h = { m, -1, 0 };
    for (int e = 1; e <= L; e++) {
        int *c = &D[(size_t)e * nr]; const int *q = &D[(size_t)(e - 1) * nr];
        c[0] = 0;
        for (int i = 1; i <= m; i++) c[i] = std::min(q[i - 1] + (p[(size_t)i - 1] != x[(size_t)e - 1] ? 1 : 0), std::min(q[i] + 1, c[i - 1] + 1));
        if (c[m] < h.dist) { h.dist = c[m]; h.end = e; }
    }
    // A(i, j) = ed(the last i bases of p, x[end - j .. end)): its row m is every s at once
    const int E = h.end;
    std::vector<int> A((size_t)(E + 1) * (size_t)nr);
    for (int i = 0; i <= m; i++) A[(size_t)i] = i;
    for (int j = 1; j <= E; j++) {
        int *c = &A[(size_t)j * nr]; const int *q = &A[(size_t)(j - 1) * nr];
        c[0] = j;
        for (int i = 1; i <= m; i++) c[i] = std::min(q[i - 1] + (p[(size_t)(m - i)] != x[(size_t)(E - j)] ? 1 : 0), std::min(q[i] + 1, c[i - 1] + 1));
    }
    for (int s = E; s >= 0 && h.start < 0; s--) if (A[(size_t)(E - s) * nr + m] == h.dist) h.start = s;
    if (each_s) {
        int want = -1;
        for (int s = 0; s <= E; s++) if (ed(p, x.data() + s, E - s) == h.dist) want = s;
        if (want != h.start) { printf("the check's own two forms of start differ: %d and %d\n", h.start, want); exit(2); }
    }
    return h;
}

struct LoadChecked {
    const std::vector<uint32_t> *w;
    uint32_t operator()(int i) const { if (i < 0 || (size_t)i >= w->size()) { printf("word %d of %zu loaded\n", i, w->size()); exit(3); } return (*w)[(size_t)i]; }
};

// the device layout of all[0 .. n): exactly the words its bases touch
static std::vector<uint32_t> pack(const Seq &all)
{
    std::vector<uint32_t> w((all.size() + 15) / 16, 0u);
    for (size_t i = 0; i < all.size(); i++) w[i >> 4] |= (uint32_t)all[i] << (30 - 2 * (int)(i & 15));
    return w;
}

static Seq edited(const Seq &p, int edits)
{
    Seq q = p;
    for (int k = 0; k < edits; k++) {
        const int at = rnd_in(0, (int)q.size() - 1), what = rnd_in(0, 2);
        if (what == 0) q[(size_t)at] = (uint8_t)((q[(size_t)at] + 1 + rnd() % 3u) & 3u);
        else if (what == 1 && q.size() > 1) q.erase(q.begin() + at);
        else q.insert(q.begin() + at, (uint8_t)(rnd() & 3u));
    }
    return q;
}
static Seq cat(const Seq &a, const Seq &b, const Seq &c) { Seq r = a; r.insert(r.end(), b.begin(), b.end()); r.insert(r.end(), c.begin(), c.end()); return r; }

static long g_cases = 0, g_equal_pairs = 0, g_inside_word = 0, g_short = 0;

template <class W>
static bool one(const Seq &p, const Seq &x, int lo, const char *what)
{
    const int m = (int)p.size(), L = (int)x.size();
    const Seq all = cat(rnd_seq(lo), x, Seq());
    const std::vector<uint32_t> words = pack(all);
    const LoadChecked ld = { &words };
    const FbvMasks<W> eq = fbv_masks<W>(p.data(), m, 0), rev = fbv_masks<W>(p.data(), m, 1);
    const FbvHit got = fbv_search<W>(ld, L, eq, rev, m, lo), want = naive(p, x, g_cases % 8 == 0);
    g_cases++;
    if (lo & 15) g_inside_word++;
    if (L < m) g_short++;
    if (got.dist != want.dist || got.end != want.end || got.start != want.start || want.end - want.start > m + want.dist) {
        printf("%s, %d-bit word, m = %d, L = %d, lo = %d: got dist %d start %d end %d, the definition says %d %d %d\n", what, (int)(8 * sizeof(W)), m, L, lo,
               got.dist, got.start, got.end, want.dist, want.start, want.end);
        return false;
    }
    return true;
}

template <class W>
static bool width(const int *lens, int n_lens, int reps)
{
    static const int edge[6] = { 15, 16, 17, 31, 32, 33 };
    for (int k = 0; k < n_lens; k++) {
        const int m = lens[k];
        for (int rep = 0; rep < reps; rep++) {
            const Seq p = rep % 5 == 4 ? Seq((size_t)m, (uint8_t)(rnd() & 3u)) : rnd_seq(m);       // (every fifth pattern one base repeated: ties everywhere)
            bool ok = true;
            switch (rep % 12) {
            case 0: ok = one<W>(p, Seq(), 0, "empty text") && one<W>(p, Seq(), rnd_in(1, 40), "empty window"); break;
            case 1: ok = one<W>(p, rnd_seq(1), 0, "one base") && one<W>(p, Seq(1, p[0]), 0, "one matching base"); break;
            case 2: ok = one<W>(p, rnd_seq(rnd_in(0, m - 1)), 0, "text shorter than the pattern") && one<W>(p, Seq(p.begin(), p.begin() + m / 2), 0, "half the pattern"); break;
            case 3: for (int t = 0; t < 6 && ok; t++) ok = one<W>(p, rnd_seq(edge[t]), 0, "a word's edge") && one<W>(p, cat(rnd_seq(std::max(0, edge[t] - m)), p, Seq()), 0, "a hit up to a word's edge"); break;
            case 4: ok = one<W>(p, cat(Seq(), edited(p, rnd_in(0, 4)), rnd_seq(rnd_in(0, 70))), 0, "a hit at the very start"); break;
            case 5: ok = one<W>(p, cat(rnd_seq(rnd_in(0, 70)), edited(p, rnd_in(0, 4)), Seq()), 0, "a hit at the very end"); break;
            case 6: {
                const Seq q = edited(p, rnd_in(0, 2)), x = cat(cat(rnd_seq(rnd_in(0, 30)), q, rnd_seq(rnd_in(1, 30))), q, rnd_seq(rnd_in(0, 30)));
                ok = one<W>(p, x, 0, "two hits of equal distance");
                g_equal_pairs++;
                break;
            }
            case 7: ok = one<W>(p, cat(rnd_seq(rnd_in(0, 40)), edited(p, rnd_in(0, 4)), rnd_seq(rnd_in(0, 40))), rnd_in(1, 15), "a window that begins inside a word")
                         && one<W>(p, edited(p, rnd_in(0, 2)), rnd_in(17, 31), "a window that is the hit"); break;
            case 8: ok = one<W>(p, rnd_seq(rnd_in(0, 150)), rnd_in(0, 33), "a random text"); break;
            default: ok = one<W>(p, cat(rnd_seq(rnd_in(0, 60)), edited(p, rnd_in(0, 4)), rnd_seq(rnd_in(0, 60))), rep % 2 ? 0 : rnd_in(0, 20), "a planted hit"); break;
            }
            if (!ok) return false;
        }
    }
    return true;
}

int main()
{
    static const int l32[4] = { 1, 2, 31, 32 }, l64[7] = { 1, 2, 31, 32, 33, 63, 64 };
    if (!width<uint32_t>(l32, 4, 720) || !width<uint64_t>(l64, 7, 720)) return 1;
    // the tie rule by hand: two exact copies, the first one's end wins, and the largest start is the copy's own
    {
        const Seq p = { 0, 1, 2, 3, 0, 1 }, gap = { 3, 3, 3, 3, 3, 3, 3 }, x = cat(cat(gap, p, gap), p, gap);
        const std::vector<uint32_t> words = pack(x);
        const LoadChecked ld = { &words };
        const FbvHit h = fbv_search<uint32_t>(ld, (int)x.size(), fbv_masks<uint32_t>(p.data(), 6, 0), fbv_masks<uint32_t>(p.data(), 6, 1), 6);
        if (h.dist != 0 || h.start != 7 || h.end != 13) { printf("two exact copies: %d %d %d\n", h.dist, h.start, h.end); return 1; }
    }
    if (g_equal_pairs < 100 || g_inside_word < 500 || g_short < 500) { printf("a degenerate run: %ld %ld %ld\n", g_equal_pairs, g_inside_word, g_short); return 1; }
    printf("%ld cases checked (%ld in windows that begin inside a word, %ld shorter than the pattern): ok\n", g_cases, g_inside_word, g_short);
    return 0;
}
