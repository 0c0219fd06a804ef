// motif_ext_check.cpp — the per-lane anchored extension of the partial genotype (mtr_amd/csrc/motif_ext.h) for the host: a program of its own (the
// form a sanitizer build runs) that compares ext_len, motif_bases, matches and score of motif_ext<UB>() with a full-matrix DP written here from
// the definition of include/mtr_hip.h ("partial genotype").  Both directions; every bucket with U at its edges (1 and 4, 5 and 8, 9 and 16, 17 and
// 32) and in between; lo and hi at all 16 residues of a word; n of 0, 1 and U - 1; six score sets, (5, 4, 7) among them; windows that are a noisy
// repeat to their end, a noisy repeat closed by other bases (the early exit's case), and random bases.  The packed text holds exactly the words
// the window touches - [lo >> 4, (hi - 1) >> 4] - and every load is checked against them, so an extension that loads beyond the window, below it or
// above, fails here and trips the address sanitizer.  The full matrix also runs with the predecessor priority reversed: enough cases must depend
// on it, or the tie rule would go untested.
#include "../mtr_amd/csrc/motif_ext.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef std::vector<uint8_t> Seq;

static uint32_t g_rng = 2024u;
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

static long g_cases = 0, g_priority = 0, g_back = 0, g_zero = 0, g_closed = 0, g_res_lo[16], g_res_hi[16];

// the window's bases in READ order (wnd = x[lo .. hi)) at lo; the motif Mo of the slot; back: the extension walks from hi downwards
template <int UB>
static bool one(const Seq &wnd, int lo, const Seq &Mo, int back, int G, int MM, int D, const char *what)
{
    const int n = (int)wnd.size(), hi = lo + n, U = (int)Mo.size();
    // exactly the words of [lo, hi); the bases of those words outside the window are random
    const int w0 = lo >> 4, w1 = n > 0 ? (hi - 1) >> 4 : w0 - 1;
    std::vector<uint32_t> words((size_t)(w1 - w0 + 1), 0u);
    for (int p = w0 * 16; p < (w1 + 1) * 16; p++) {
        const uint32_t c = p >= lo && p < hi ? wnd[(size_t)(p - lo)] : (rnd() & 3u);
        words[(size_t)((p >> 4) - w0)] |= c << (30 - 2 * (p & 15));
    }
    const LoadChecked ld = { &words, w0 };
    Seq y = wnd, m = Mo;
    if (back) { std::reverse(y.begin(), y.end()); std::reverse(m.begin(), m.end()); }
    const MotifExt got = motif_ext<UB>(ld, lo, hi, back, mdp_motif_bits(m.data(), U), U, G, MM, D);
    const MotifExt want = naive(y, m, G, MM, D, false), other = naive(y, m, G, MM, D, true);
    g_cases++;
    if (other.motif_bases != want.motif_bases || other.matches != want.matches) g_priority++;
    if (back) g_back++;
    if (want.score == 0) g_zero++;
    if (want.ext_len > 0 && want.ext_len + 16 < n) g_closed++;
    g_res_lo[lo & 15]++; g_res_hi[hi & 15]++;
    if (got.ext_len != want.ext_len || got.motif_bases != want.motif_bases || got.matches != want.matches || got.score != want.score) {
        printf("%s, UB = %d, U = %d, n = %d, lo = %d, back = %d, scores %d %d %d: got len %d bases %d matches %d score %d, the definition says %d %d %d %d\n", what, UB, U, n, lo,
               back, G, MM, D, got.ext_len, got.motif_bases, got.matches, got.score, want.ext_len, want.motif_bases, want.matches, want.score);
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
            int want_hi = (rep / 16) % 16;                           // hi at every residue as well: the window's length is made to fit
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
    static const int u4[4] = { 1, 2, 3, 4 }, u8[3] = { 5, 7, 8 }, u16[3] = { 9, 12, 16 }, u32[3] = { 17, 25, 32 };
    if (!bucket<4>(u4, 4, 960) || !bucket<8>(u8, 3, 960) || !bucket<16>(u16, 3, 960) || !bucket<32>(u32, 3, 960)) return 1;
    // by hand (include/mtr_hip.h's rules): CAA against AA - the C is a mismatch, not an insertion: three motif bases, two matches, score 1
    {
        const Seq w = { 1, 0, 0 }, M = { 0, 0 };
        std::vector<uint32_t> words(1, 0u);
        for (int p = 0; p < 3; p++) words[0] |= (uint32_t)w[(size_t)p] << (30 - 2 * p);
        const LoadChecked ld = { &words, 0 };
        const MotifExt r = motif_ext<4>(ld, 0, 3, 0, mdp_motif_bits(M.data(), 2), 2, 1, 1, 1);
        if (r.ext_len != 3 || r.motif_bases != 3 || r.matches != 2 || r.score != 1) { printf("CAA against AA: %d %d %d %d\n", r.ext_len, r.motif_bases, r.matches, r.score); return 1; }
    }
    bool residues = true;
    for (int r = 0; r < 16; r++) residues = residues && g_res_lo[r] >= 100 && g_res_hi[r] >= 100;
    if (!residues || g_priority < 300 || g_back < 4000 || g_zero < 300 || g_closed < 300) {
        printf("a degenerate run: residues %d, %ld depend on the priority, %ld backward, %ld without a positive cell, %ld closed\n", (int)residues, g_priority, g_back, g_zero, g_closed);
        return 1;
    }
    printf("%ld cases checked (%ld backward, %ld depend on the predecessor priority, %ld without a positive cell, %ld closed well before the window's end): ok\n", g_cases, g_back,
           g_priority, g_zero, g_closed);
    return 0;
}
