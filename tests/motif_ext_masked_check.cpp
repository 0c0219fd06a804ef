// motif_ext_masked_check.cpp — the MASKED rows of the per-lane anchored extension (mtr_amd/csrc/motif_ext.h: motif_ext_rows<UB, false>) for the
// host: a program of its own (the form a sanitizer build runs).  The partial genotype at catalogue scale (partial_catalog.hip.inc) gives every
// lane a motif, a length and a direction of its own and so calls the masked rows for EVERY U <= UB, U == UB included - the case motif_ext<UB>()
// hands to the rows compiled without a cut, which tests/motif_ext_check.cpp therefore never runs masked.  Here, per bucket and in both directions:
// U == UB masked against the uncut rows and against a full-matrix DP written from the definition of include/mtr_hip.h ("partial genotype"); and
// every U <= UB masked against the full matrix, as tests/motif_ext_check.cpp covers it through the dispatch.  lo and hi at all 16 residues of a
// word; windows of 0, 1 and U - 1 bases, random bases, noisy repeats to the window's end and closed ones; six score sets.  The packed text holds
// exactly the words the window touches and every load is checked against them.  The full matrix also runs with the predecessor priority reversed:
// enough cases must depend on it.
#include "../mtr_amd/csrc/motif_ext.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef std::vector<uint8_t> Seq;

static uint32_t g_rng = 4051u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }      // lo .. hi
static Seq rnd_seq(int n) { Seq s((size_t)n); for (auto &v : s) v = (uint8_t)(rnd() & 3u); return s; }

struct Cell { int H, C, T; };

// the definition on y[0 .. n) against m[0 .. U); reversed: the predecessor is the LAST of sub, left, up that attains H
static MotifExt naive(const Seq &y, const Seq &m, int G, int MM, int D, bool reversed)
{
    const int n = (int)y.size(), U = (int)m.size();
    std::vector<Cell> mat((size_t)(n + 1) * (size_t)(U + 1), Cell{ 0, 0, 0 });
    MotifExt best = { 0, 0, 0, 0 };
    for (int i = 1; i <= n; i++) {
        Cell *cur = &mat[(size_t)i * (size_t)(U + 1)]; const Cell *prev = &mat[(size_t)(i - 1) * (size_t)(U + 1)];
        for (int j = 1; j <= U; j++) {
            const bool match = y[(size_t)i - 1] == m[(size_t)j - 1];
            const Cell d = prev[j - 1];                                 // (column 0 holds column U)
            Cell cand[3]; int nc = 0;
            cand[nc++] = Cell{ d.H + (match ? G : -MM), d.C + 1, d.T + (match ? 1 : 0) };
            if (j > 1) cand[nc++] = Cell{ cur[j - 1].H - D, cur[j - 1].C + 1, cur[j - 1].T };
            cand[nc++] = Cell{ prev[j].H - D, prev[j].C, prev[j].T };
            int h = cand[0].H;
            for (int k = 1; k < nc; k++) h = std::max(h, cand[k].H);
            int pick = -1;
            for (int k = 0; k < nc; k++) if (cand[k].H == h && (pick < 0 || reversed)) pick = k;
            cur[j] = cand[pick];
            if (h > best.score) best = MotifExt{ i, cur[j].C, cur[j].T, h };
        }
        cur[0] = cur[U];
    }
    return best;
}

struct LoadChecked {
    const std::vector<uint32_t> *w; int w0;
    uint32_t operator()(int i) const
    {
        if (i < w0 || (size_t)(i - w0) >= w->size()) { printf("word %d loaded, the window holds %d .. %d\n", i, w0, w0 + (int)w->size() - 1); exit(3); }
        return (*w)[(size_t)(i - w0)];
    }
};

static Seq edited(const Seq &p, int edits)
{
    Seq q = p;
    for (int k = 0; k < edits && !q.empty(); k++) {
        const int at = rnd_in(0, (int)q.size() - 1), what = rnd_in(0, 2);
        if (what == 0) q[(size_t)at] = (uint8_t)((q[(size_t)at] + 1 + rnd() % 3u) & 3u);
        else if (what == 1 && q.size() > 1) q.erase(q.begin() + at);
        else q.insert(q.begin() + at, (uint8_t)(rnd() & 3u));
    }
    return q;
}

static bool same(const MotifExt &a, const MotifExt &b) { return a.ext_len == b.ext_len && a.motif_bases == b.motif_bases && a.matches == b.matches && a.score == b.score; }

static long g_cases = 0, g_full = 0, g_priority = 0, g_back = 0, g_zero = 0, g_closed = 0, g_res_lo[16], g_res_hi[16];

// the window's bases in READ order (wnd = x[lo .. hi)) at lo; the motif Mo of the slot; back: the extension walks from hi downwards
template <int UB>
static bool one(const Seq &wnd, int lo, const Seq &Mo, int back, int G, int MM, int D, const char *what)
{
    const int n = (int)wnd.size(), hi = lo + n, U = (int)Mo.size();
    const int w0 = lo >> 4, w1 = n > 0 ? (hi - 1) >> 4 : w0 - 1;
    std::vector<uint32_t> words((size_t)(w1 - w0 + 1), 0u);
    for (int p = w0 * 16; p < (w1 + 1) * 16; p++) {
        const uint32_t c = p >= lo && p < hi ? wnd[(size_t)(p - lo)] : (rnd() & 3u);
        words[(size_t)((p >> 4) - w0)] |= c << (30 - 2 * (p & 15));
    }
    const LoadChecked ld = { &words, w0 };
    Seq y = wnd, m = Mo;
    if (back) { std::reverse(y.begin(), y.end()); std::reverse(m.begin(), m.end()); }
    // the bits above the motif's are not the lane's business: fill them, the masked rows must not read them into a result
    uint64_t bits = mdp_motif_bits(m.data(), U);
    if (U < 32) bits |= ((uint64_t)rnd() << 40 | (uint64_t)rnd() << 16 | rnd()) << (2 * U);
    const MotifExt got = motif_ext_rows<UB, false>(ld, lo, hi, back, bits, U, G, MM, D);
    const MotifExt want = naive(y, m, G, MM, D, false), other = naive(y, m, G, MM, D, true);
    g_cases++;
    if (other.motif_bases != want.motif_bases || other.matches != want.matches) g_priority++;
    if (back) g_back++;
    if (want.score == 0) g_zero++;
    if (want.ext_len > 0 && want.ext_len + 16 < n) g_closed++;
    g_res_lo[lo & 15]++; g_res_hi[hi & 15]++;
    bool ok = same(got, want);
    MotifExt uncut = want;
    if (U == UB) { uncut = motif_ext_rows<UB, true>(ld, lo, hi, back, bits, U, G, MM, D); g_full++; ok = ok && same(got, uncut); }
    if (!ok) {
        printf("%s, UB = %d, U = %d, n = %d, lo = %d, back = %d, scores %d %d %d: masked len %d bases %d matches %d score %d, the definition says %d %d %d %d, the uncut rows %d %d %d %d\n",
               what, UB, U, n, lo, back, G, MM, D, got.ext_len, got.motif_bases, got.matches, got.score, want.ext_len, want.motif_bases, want.matches, want.score,
               uncut.ext_len, uncut.motif_bases, uncut.matches, uncut.score);
        return false;
    }
    return true;
}

static Seq tandem(const Seq &M, int phase, int len)
{
    Seq r((size_t)len);
    for (int t = 0; t < len; t++) r[(size_t)t] = M[(size_t)((phase + t) % (int)M.size())];
    return r;
}

template <int UB>
static bool bucket(const int *us, int n_us, int reps)
{
    static const int scores[6][3] = { { 1, 1, 1 }, { 2, 3, 2 }, { 5, 4, 7 }, { 5, 1, 1 }, { 1, 1, 3 }, { 1, 3, 1 } };
    for (int k = 0; k < n_us; k++) {
        const int U = us[k];
        for (int rep = 0; rep < reps; rep++) {
            const Seq M = rep % 7 == 6 ? Seq((size_t)U, (uint8_t)(rnd() & 3u)) : rnd_seq(U);
            const int *s = scores[rep % 6], back = (rep / 6) & 1, lo = (rep % 16) + 16 * rnd_in(0, 3);
            const int len = rnd_in(1, 120);
            const int want_hi = (rep / 16) % 16;                     // hi at every residue as well: the window's length is made to fit
            int n = len; while (((lo + n) & 15) != want_hi) n++;
            bool ok = true;
            switch (rep % 10) {
            case 0: ok = one<UB>(Seq(), lo, M, back, s[0], s[1], s[2], "an empty window"); break;
            case 1: ok = one<UB>(rnd_seq(1), lo, M, back, s[0], s[1], s[2], "one base") && one<UB>(Seq(1, M[0]), lo, M, back, s[0], s[1], s[2], "one matching base"); break;
            case 2: ok = one<UB>(tandem(M, rnd_in(0, U - 1), U - 1), lo, M, back, s[0], s[1], s[2], "a window of U - 1 bases"); break;
            case 3: ok = one<UB>(rnd_seq(n), lo, M, back, s[0], s[1], s[2], "random bases"); break;
            case 4: case 5: {                                        // a noisy repeat closed by other bases: the repeat lies at the extension's start
                const int rl = rnd_in(1, n);
                Seq rp = edited(tandem(M, rnd_in(0, U - 1), rl), rl / 10), rest = rnd_seq(n);
                rp.resize((size_t)std::min<int>((int)rp.size(), n));
                Seq w = back ? Seq(rest.begin(), rest.begin() + (n - (int)rp.size())) : rp;
                if (back) w.insert(w.end(), rp.begin(), rp.end()); else w.insert(w.end(), rest.begin(), rest.begin() + (n - (int)rp.size()));
                ok = one<UB>(w, lo, M, back, s[0], s[1], s[2], "a closed repeat");
                break;
            }
            default: {
                Seq w = edited(tandem(M, rnd_in(0, U - 1), n), n / rnd_in(6, 30));
                if ((int)w.size() < n) { const Seq more = tandem(M, 0, n - (int)w.size()); w.insert(w.end(), more.begin(), more.end()); }
                w.resize((size_t)n);
                ok = one<UB>(w, lo, M, back, s[0], s[1], s[2], "a noisy repeat to the window's end");
                break;
            }
            }
            if (!ok) return false;
        }
    }
    return true;
}

int main()
{
    // U == UB comes first and most often: it is what the dispatch never runs masked
    static const int u4[4] = { 4, 1, 2, 3 }, u8[4] = { 8, 5, 7, 8 }, u16[4] = { 16, 9, 12, 16 }, u32[4] = { 32, 17, 25, 32 };
    if (!bucket<4>(u4, 4, 800) || !bucket<8>(u8, 4, 800) || !bucket<16>(u16, 4, 800) || !bucket<32>(u32, 4, 800)) return 1;
    bool residues = true;
    for (int r = 0; r < 16; r++) residues = residues && g_res_lo[r] >= 100 && g_res_hi[r] >= 100;
    if (!residues || g_full < 4000 || g_priority < 300 || g_back < 4000 || g_zero < 300 || g_closed < 300) {
        printf("a degenerate run: residues %d, %ld with U == UB, %ld depend on the priority, %ld backward, %ld without a positive cell, %ld closed\n", (int)residues, g_full, g_priority,
               g_back, g_zero, g_closed);
        return 1;
    }
    printf("%ld cases checked (%ld with U == UB against the uncut rows too, %ld backward, %ld depend on the predecessor priority, %ld without a positive cell, %ld closed well before "
           "the window's end): ok\n", g_cases, g_full, g_back, g_priority, g_zero, g_closed);
    return 0;
}
