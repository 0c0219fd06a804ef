// window_structure_check.cpp — the window structure's sequential function (mtr_amd/csrc/window_structure.h: ws_rows, the code the gfx950 lanes run)
// as a program of its own (the form a sanitizer build runs), against a brute force written here from include/mtr_hip.h's definition: the full
// matrix, every row iterated until nothing changes (so that "two sweeps suffice" is tested, not assumed), each cell's predecessor stored - the
// first candidate of the definition's order that attains the maximum - and copies, matches and entries counted along the traceback from the end.
// The window is a heap buffer of exactly n bytes placed at every residue of the 8-byte load: the loader refuses a word that holds none of its
// bytes, hands out a poison byte for the positions of a word outside the window, and the address sanitizer sees every read of the buffer.
//   window_structure_check [cases]           the check (default 12 000 seeded cases); prints "ok: ..." and exits 0, or the first difference and 1
//   window_structure_check --time FILE       one thread over the windows of FILE (N windows of LEN bases, structure 0: CAG, or 1: CAG CAA CCGCCA CCG):
//                                            prints the milliseconds and the scores' sum (the yardstick of tests/dev/gpu_window_structure.py)
#include "../mtr_amd/csrc/window_structure.h"

#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }      // xorshift32
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

typedef std::vector<std::vector<uint8_t>> Structure;        // motifs as codes

static WsStruct pack(const Structure &ms)
{
    WsStruct st = { 0, 0, 0, 0, 0, (int32_t)ms.size() };
    int c = 0;
    for (size_t s = 0; s < ms.size(); s++) {
        st.first |= 1u << c;
        for (uint8_t b : ms[s]) { st.mot |= (uint64_t)b << (2 * c); st.seg |= (uint64_t)s << (2 * c); c++; }
        st.last |= 1u << (c - 1);
    }
    st.W = c;
    return st;
}

// ---- the brute force ----
static const int NONE = INT_MIN / 4;
struct Brute { int score; int32_t seg[16]; int matches; };
static Brute brute(const Structure &ms, const uint8_t *y, int n, int G, int MM, int D)
{
    const int S = (int)ms.size();
    std::vector<int> m, sg, first(S), last(S);
    for (int s = 0; s < S; s++) { first[s] = (int)m.size(); for (uint8_t b : ms[s]) { m.push_back(b); sg.push_back(s); } last[s] = (int)m.size() - 1; }
    const int W = (int)m.size(), START = W;
    std::vector<std::vector<int>> preds(W);
    for (int c = 0; c < W; c++) {
        const int s = sg[c];
        if (c != first[s]) preds[c].push_back(c - 1);
        else { for (int t = s - 1; t >= 0; t--) preds[c].push_back(last[t]); preds[c].push_back(START); preds[c].push_back(last[s]); }
    }
    struct Cell { int h, kind, p; };                     // kind 0 sub, 1 up, 2 left, -1 none
    std::vector<std::vector<Cell>> T((size_t)n + 1, std::vector<Cell>((size_t)W + 1, Cell{ NONE, -1, -1 }));
    for (int i = 0; i <= n; i++) {
        T[i][START] = Cell{ -D * i, -1, -1 };
        for (bool changed = true; changed;) {
            changed = false;
            for (int c = 0; c < W; c++) {
                Cell best{ NONE, -1, -1 };
                if (i >= 1) for (int p : preds[c]) if (T[i - 1][p].h != NONE) { const int v = T[i - 1][p].h + (y[i - 1] == m[c] ? G : -MM); if (v > best.h) best = Cell{ v, 0, p }; }
                if (i >= 1 && T[i - 1][c].h != NONE) { const int v = T[i - 1][c].h - D; if (v > best.h) best = Cell{ v, 1, c }; }
                for (int p : preds[c]) if (T[i][p].h != NONE) { const int v = T[i][p].h - D; if (v > best.h) best = Cell{ v, 2, p }; }
                if (best.h != T[i][c].h || best.kind != T[i][c].kind || best.p != T[i][c].p) { T[i][c] = best; changed = true; }
            }
        }
    }
    int e = -1, eh = NONE;
    for (int s = S - 1; s >= 0; s--) if (T[n][last[s]].h > eh) { eh = T[n][last[s]].h; e = last[s]; }
    if (T[n][START].h > eh) { eh = T[n][START].h; e = START; }
    int copies[4] = { 0, 0, 0, 0 }, matches[4] = { 0, 0, 0, 0 }, entry[4] = { 0, 0, 0, 0 };
    for (int i = n, c = e; c != START;) {
        const Cell &x = T[i][c];
        const int s = sg[c];
        if (x.kind != 1) {
            if (c == last[s]) copies[s]++;
            if (x.kind == 0 && y[i - 1] == m[c]) matches[s]++;
            if (c == first[s] && x.p != last[s]) entry[s] = x.kind == 0 ? i - 1 : i;
        }
        if (x.kind == 0) { i--; c = x.p; } else if (x.kind == 1) i--; else c = x.p;
    }
    Brute out; out.score = eh; out.matches = 0; memset(out.seg, 0, sizeof out.seg);
    int nxt = n;
    for (int s = S - 1; s >= 0; s--) {
        int32_t *o = out.seg + 4 * s;
        if (copies[s] > 0) { o[0] = entry[s]; o[1] = nxt; o[2] = copies[s]; o[3] = matches[s]; nxt = entry[s]; }
        else { o[0] = nxt; o[1] = nxt; }
        out.matches += matches[s];
    }
    return out;
}

// ---- the window at a residue of the load ----
struct Window {
    uint8_t *buf; int n, r; long *loads;
    uint64_t operator()(int k) const
    {
        if (k < 0 || (n > 0 && k > (r + n - 1) >> 3) || n == 0) { fprintf(stderr, "FAIL: word %d asked for, the window of %d bases at residue %d has none of it\n", k, n, r); exit(1); }
        ++*loads;
        uint64_t w = 0;
        for (int b = 0; b < 8; b++) { const int p = 8 * k + b - r; w |= (uint64_t)(p >= 0 && p < n ? buf[p] : 0xEE) << (8 * b); }
        return w;
    }
};

template <int UB, bool WIDE> static WsRaw run(const Window &w, const WsStruct &st, int G, int MM, int D) { return ws_rows<UB, WIDE>(w, w.r, w.n, st, G, MM, D); }
typedef WsRaw (*RunFn)(const Window &, const WsStruct &, int, int, int);
static const struct { int ub; bool wide; RunFn fn; const char *name; } INST[5] = {
    { 8, false, run<8, false>, "<8, narrow>" }, { 16, false, run<16, false>, "<16, narrow>" }, { 32, false, run<32, false>, "<32, narrow>" },
    { 8, true, run<8, true>, "<8, wide>" }, { 16, true, run<16, true>, "<16, wide>" } };

static std::string show(const Structure &ms, const uint8_t *y, int n)
{
    std::string s = "[";
    for (const auto &mo : ms) { for (uint8_t b : mo) s += "ACGT"[b]; s += ' '; }
    s += "] ";
    for (int i = 0; i < n; i++) s += "ACGT"[y[i]];
    return s;
}

static const int SCORES[6][3] = { { 1, 1, 1 }, { 2, 3, 2 }, { 5, 1, 1 }, { 1, 3, 3 }, { 3, 2, 1 }, { 2, 1, 3 } };
static const int W_NARROW[] = { 1, 2, 7, 8, 9, 15, 16, 17, 31, 32 }, W_WIDE[] = { 3, 4, 7, 8, 9, 15, 16 };

static Structure random_structure(int S, int W, int alphabet)
{
    std::vector<int> len((size_t)S, 1);
    for (int k = S; k < W; k++) len[(size_t)rnd_in(0, S - 1)]++;
    Structure ms;
    for (int s = 0; s < S; s++) { ms.emplace_back(); for (int t = 0; t < len[(size_t)s]; t++) ms.back().push_back((uint8_t)rnd_in(0, alphabet - 1)); }
    return ms;
}
// copies of the motifs in order with errors at `rate` percent, or plain noise
static std::vector<uint8_t> random_window(const Structure &ms, int n, int rate, int alphabet)
{
    std::vector<uint8_t> y;
    if (rnd_in(0, 5) == 0) { for (int i = 0; i < n; i++) y.push_back((uint8_t)rnd_in(0, alphabet - 1)); return y; }
    for (size_t s = 0; s < ms.size() && (int)y.size() < n + 8; s++)
        for (int k = rnd_in(0, 1 + n / (int)(ms[s].size() * ms.size())); k > 0; k--)
            for (uint8_t b : ms[s]) {
                const int e = rnd_in(0, 99) < rate ? rnd_in(0, 2) : 3;
                if (e == 0) y.push_back((uint8_t)rnd_in(0, alphabet - 1));                      // a substitution
                else if (e == 1) { y.push_back(b); y.push_back((uint8_t)rnd_in(0, alphabet - 1)); }   // an insertion
                else if (e == 3) y.push_back(b);                                                // (e == 2: a deletion)
            }
    while ((int)y.size() < n) y.push_back((uint8_t)rnd_in(0, alphabet - 1));
    y.resize((size_t)n);
    return y;
}

// FILE: int32 N, LEN, K, then N * LEN codes - the windows the GPU was given (tests/dev/gpu_window_structure.py writes it)
static int time_mode(const char *path)
{
    FILE *f = fopen(path, "rb");
    int32_t head[3] = { 0, 0, 0 };
    if (!f || fread(head, 4, 3, f) != 3 || head[0] < 0 || head[1] < 1 || head[1] > WS_MAX_WINDOW) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    const int N = head[0], len = head[1], kind = head[2];
    const Structure ms = kind == 0 ? Structure{ { 1, 0, 2 } } : Structure{ { 1, 0, 2 }, { 1, 0, 0 }, { 1, 1, 2, 1, 1, 0 }, { 1, 1, 2 } };
    const WsStruct st = pack(ms);
    std::vector<uint8_t> all((size_t)N * (size_t)len + 8);                                               // 8 bytes of head room: plain aligned loads, as the lanes do
    if (fread(all.data(), 1, (size_t)N * (size_t)len, f) != (size_t)N * (size_t)len) { fprintf(stderr, "%s is short\n", path); return 2; }
    fclose(f);
    long sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int w = 0; w < N; w++) {
        const uint8_t *at = all.data() + (size_t)w * (size_t)len;
        const int r = (int)((uintptr_t)at & 7);
        const auto ld = [at, r](int k) { uint64_t v; memcpy(&v, at - r + 8 * k, 8); return v; };
        const WsRaw raw = kind == 0 ? ws_rows<8, false>(ld, r, len, st, 1, 1, 1) : ws_rows<16, true>(ld, r, len, st, 1, 1, 1);
        sum += raw.score;
    }
    const double ms_taken = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"windows\": %d, \"bases\": %d, \"structure\": %d, \"host_ms\": %.3f, \"score_sum\": %ld}\n", N, len, kind, ms_taken, sum);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "--time")) return time_mode(argv[2]);
    const long cases = argc > 1 ? atol(argv[1]) : 12000;
    long runs = 0, loads = 0, wraps = 0, skipped_segments = 0, start_ends = 0;
    for (long t = 0; t < cases; t++) {
        const bool wide = t % 3 == 2;
        const int W = wide ? W_WIDE[(t / 3) % 7] : W_NARROW[(t / 3) % 10];
        const int S = wide ? rnd_in(3, W < 4 ? 3 : 4) : rnd_in(1, W < 2 ? 1 : 2);
        const int *sc = SCORES[(t / 7) % 6];
        const int alphabet = rnd_in(1, 4), r = (int)(t % 8);
        const Structure ms = random_structure(S, W, alphabet);
        const int U0 = (int)ms[0].size();
        const int pick = (int)((t / 5) % 6);
        const int n = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? U0 - 1 : rnd_in(2, W <= 8 ? 40 : 70);
        const std::vector<uint8_t> y = random_window(ms, n, (int)((t / 11) % 3) * 12, alphabet);
        uint8_t *buf = (uint8_t *)malloc((size_t)(n > 0 ? n : 1));                           // exactly the window: a read beyond it is the sanitizer's
        if (n > 0) memcpy(buf, y.data(), (size_t)n);
        const Brute want = brute(ms, buf, n, sc[0], sc[1], sc[2]);
        const WsStruct st = pack(ms);
        for (const auto &in : INST) {
            if (in.ub < W || (!in.wide && S > 2)) continue;
            if (n == 0) continue;                                                               // (no DP: the caller's zeros, checked below)
            const Window w = { buf, n, r, &loads };
            const WsRaw raw = in.fn(w, st, sc[0], sc[1], sc[2]);
            int32_t seg[16];
            ws_spans(raw, n, S, seg);
            runs++;
            if (raw.score != want.score || memcmp(seg, want.seg, sizeof seg) || ws_matches(raw) != want.matches) {
                fprintf(stderr, "FAIL: case %ld %s scores (%d, %d, %d) residue %d: %s\n  header: score %d seg", t, in.name, sc[0], sc[1], sc[2], r, show(ms, buf, n).c_str(), raw.score);
                for (int k = 0; k < 16; k++) fprintf(stderr, " %d", seg[k]);
                fprintf(stderr, "\n  brute:  score %d seg", want.score);
                for (int k = 0; k < 16; k++) fprintf(stderr, " %d", want.seg[k]);
                fprintf(stderr, "\n");
                return 1;
            }
        }
        if (n == 0 && (want.score != 0 || want.matches != 0)) { fprintf(stderr, "FAIL: the brute force of an empty window is not zeros\n"); return 1; }
        bool any = false;
        for (int s = 0; s < S; s++) { if (want.seg[4 * s + 2] == 0) skipped_segments++; else any = true; if (want.seg[4 * s + 2] > 1) wraps++; }
        if (!any) start_ends++;
        free(buf);
    }
    if (runs < 10000 || wraps == 0 || skipped_segments == 0 || start_ends == 0) { fprintf(stderr, "FAIL: the cases are degenerate: %ld runs, %ld wraps, %ld skipped segments, %ld START ends\n", runs, wraps, skipped_segments, start_ends); return 1; }
    printf("ok: %ld cases, %ld runs of ws_rows, %ld word loads\n", cases, runs, loads);
    return 0;
}
