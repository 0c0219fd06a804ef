// window_edits_check.cpp — the window edits' sequential functions (mtr_amd/csrc/window_edits.h: we_rows and we_walk, the code the gfx950 lanes run)
// as a program of its own (the form a sanitizer build runs), against a brute force written here from include/mtr_hip.h's definition ("window
// edits"): the full matrix, every row iterated until nothing changes, each cell's predecessor stored, the path read FORWARD from START to the end
// with the copy index counted as the definition counts it.  Held to it: the edit list of the counting walk plus the emitting walk, the walk's
// carried fields against we_rows' own, we_rows' result against ws_rows' bit for bit (the window structure's function is the yardstick of the
// per-window columns), and the two invariants.  The stored rows go through we_pack / we_unpack into a buffer of exactly (n + 1) * words words;
// the window is a heap buffer of exactly n bytes at every residue of the 8-byte load.
// An empty window runs neither function - the call gives its zeros without a DP, on the device too - and is held to the brute force's zeros only.
//   window_edits_check [cases]           the check (default 12 000 seeded cases); prints "ok: ..." and exits 0, or the first difference and 1
//   window_edits_check --time FILE       one thread over the windows of FILE (the format of window_structure_check --time): rows, counting walk,
//                                        emitting walk; prints the milliseconds and the edits' sum (the yardstick of tests/dev/gpu_window_edits.py)
#include "../mtr_amd/csrc/window_edits.h"

#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

typedef std::vector<std::vector<uint8_t>> Structure;

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
struct Brute { int score; int32_t seg[16]; std::vector<int32_t> edits; long ups_on_last, wrap_lefts, row0_lefts; };
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
    struct Step { int i, c, kind, p; };
    std::vector<Step> path;                              // back from the end, then read forward
    for (int i = n, c = e; c != START;) {
        const Cell &x = T[i][c];
        path.push_back(Step{ i, c, x.kind, x.p });
        if (x.kind == 0) { i--; c = x.p; } else if (x.kind == 1) i--; else c = x.p;
    }
    Brute out; out.score = eh; out.ups_on_last = out.wrap_lefts = out.row0_lefts = 0; memset(out.seg, 0, sizeof out.seg);
    int copies[4] = { 0, 0, 0, 0 }, matches[4] = { 0, 0, 0, 0 }, entry[4] = { 0, 0, 0, 0 }, landings[4] = { 0, 0, 0, 0 };
    for (size_t k = path.size(); k-- > 0;) {
        const Step &x = path[k];
        const int s = sg[x.c];
        if (x.kind != 1) {
            if (x.c == first[s]) landings[s]++;
            if (x.c == last[s]) copies[s]++;
            if (x.kind == 0 && y[x.i - 1] == m[x.c]) matches[s]++;
            if (x.c == first[s] && x.p != last[s]) entry[s] = x.kind == 0 ? x.i - 1 : x.i;
        }
        const int copy = landings[s] - 1, col = x.c - first[s];
        if (x.kind == 0 && y[x.i - 1] != m[x.c]) for (int v : { x.i - 1, s, copy, col, 0, (int)y[x.i - 1] }) out.edits.push_back(v);
        if (x.kind == 1) { for (int v : { x.i - 1, s, copy, col, 1, (int)y[x.i - 1] }) out.edits.push_back(v); if (x.c == last[s]) out.ups_on_last++; }
        if (x.kind == 2) {
            for (int v : { x.i, s, copy, col, 2, m[x.c] }) out.edits.push_back(v);
            if (x.c == first[s] && x.p == last[s]) out.wrap_lefts++;
            if (x.i == 0) out.row0_lefts++;
        }
    }
    int nxt = n;
    for (int s = S - 1; s >= 0; s--) {
        int32_t *o = out.seg + 4 * s;
        if (copies[s] > 0) { o[0] = entry[s]; o[1] = nxt; o[2] = copies[s]; o[3] = matches[s]; nxt = entry[s]; }
        else { o[0] = nxt; o[1] = nxt; }
    }
    return out;
}

// ---- the window at a residue of the load ----
struct Window {
    uint8_t *buf; int n, r;
    uint64_t operator()(int k) const
    {
        if (k < 0 || (n > 0 && k > (r + n - 1) >> 3) || n == 0) { fprintf(stderr, "FAIL: word %d asked for, the window of %d bases at residue %d has none of it\n", k, n, r); exit(1); }
        uint64_t w = 0;
        for (int b = 0; b < 8; b++) { const int p = 8 * k + b - r; w |= (uint64_t)(p >= 0 && p < n ? buf[p] : 0xEE) << (8 * b); }
        return w;
    }
};

// what the header's functions give for one window: the rows into exactly (n + 1) * words words, the counting walk, the emitting walk
struct Got { WsRaw raw, plain; WeCount count, emit; int end_id; std::vector<int32_t> edits; };
template <int UB, bool WIDE, bool MEM> static Got run(const Window &w, const WsStruct &st, int G, int MM, int D)
{
    const int NW = we_row_words(UB), n = w.n;
    uint32_t *rows = (uint32_t *)malloc((size_t)(n + 1) * (size_t)NW * 4);
    Got g;
    g.end_id = -1;
    const auto sink = [rows, NW](int i, const WeRow &rec) { for (int k = 0; k < NW; k++) rows[(size_t)i * NW + k] = we_pack(UB, rec, k); };
    if (MEM) {                                            // the previous row in memory of exactly W columns, the loops not unrolled (the device's form for the two widest buckets)
        typedef typename WsCnt<WIDE>::type P;
        int *mh = (int *)malloc((size_t)st.W * sizeof(int)); P *me = (P *)malloc((size_t)st.W * sizeof(P)), *mc = (P *)malloc((size_t)st.W * sizeof(P)), *mm = (P *)malloc((size_t)st.W * sizeof(P));
        WeRowMem<P> row = { mh, me, mc, mm, 1 };
        g.raw = we_rows_in<UB, WIDE>(row, w, sink, w.r, n, st, G, MM, D, g.end_id);
        free(mh); free(me); free(mc); free(mm);
    } else
        g.raw = we_rows<UB, WIDE>(w, sink, w.r, n, st, G, MM, D, g.end_id);
    g.plain = ws_rows<UB, WIDE>(w, w.r, n, st, G, MM, D);
    const auto row = [rows, NW, n](int i) {
        if (i < 0 || i > n) { fprintf(stderr, "FAIL: row %d asked for, the window has rows 0 .. %d\n", i, n); exit(1); }
        const uint32_t *p = rows + (size_t)i * NW;
        return we_unpack(UB, p[0], NW > 1 ? p[1] : 0u, NW > 2 ? p[2] : 0u);
    };
    const uint8_t *y = w.buf;
    const auto base = [y](int p) { return y[p]; };
    g.count = we_walk<false>(row, base, n, st, g.end_id, 0ull, 0, nullptr);
    int32_t *list = (int32_t *)malloc((size_t)(g.count.edits > 0 ? g.count.edits : 1) * WE_FIELDS * 4);     // exactly the counted edits: a write beyond them is the sanitizer's
    g.emit = we_walk<true>(row, base, n, st, g.end_id, g.count.copies, g.count.edits, list + (size_t)g.count.edits * WE_FIELDS);
    g.edits.assign(list, list + (size_t)g.count.edits * WE_FIELDS);
    free(list); free(rows);
    return g;
}
typedef Got (*RunFn)(const Window &, const WsStruct &, int, int, int);
static const struct { int ub; bool wide; RunFn fn; const char *name; } INST[7] = {
    { 8, false, run<8, false, false>, "<8, narrow>" }, { 16, false, run<16, false, false>, "<16, narrow>" }, { 32, false, run<32, false, false>, "<32, narrow>" },
    { 8, true, run<8, true, false>, "<8, wide>" }, { 16, true, run<16, true, false>, "<16, wide>" },
    { 32, false, run<32, false, true>, "<32, narrow> in memory" }, { 16, true, run<16, true, true>, "<16, wide> in memory" } };

static std::string show(const Structure &ms, const uint8_t *y, int n)
{
    std::string s = "[";
    for (const auto &mo : ms) { for (uint8_t b : mo) s += "ACGT"[b]; s += ' '; }
    s += "] ";
    for (int i = 0; i < n; i++) s += "ACGT"[y[i]];
    return s;
}
static std::string rows_of(const std::vector<int32_t> &e)
{
    std::string s;
    for (size_t k = 0; k < e.size(); k++) s += (k % WE_FIELDS ? "," : " (") + std::to_string(e[k]) + (k % WE_FIELDS == WE_FIELDS - 1 ? ")" : "");
    return s.empty() ? " none" : s;
}

static const int SCORES[6][3] = { { 1, 1, 1 }, { 2, 3, 2 }, { 5, 1, 1 }, { 1, 3, 3 }, { 3, 2, 1 }, { 2, 1, 3 } };
static const int W_NARROW[] = { 1, 2, 7, 8, 9, 15, 16, 17, 31, 32 }, W_WIDE[] = { 3, 4, 7, 8, 9, 15, 16 };
static const int N_EDGES[] = { 7, 8, 9, 15, 16, 17, 31, 32, 33 };           // either side of the window's 8-byte loads; a stored row is whole words, so rows have no boundary of their own

static Structure random_structure(int S, int W, int alphabet)
{
    std::vector<int> len((size_t)S, 1);
    for (int k = S; k < W; k++) len[(size_t)rnd_in(0, S - 1)]++;
    Structure ms;
    for (int s = 0; s < S; s++) { ms.emplace_back(); for (int t = 0; t < len[(size_t)s]; t++) ms.back().push_back((uint8_t)rnd_in(0, alphabet - 1)); }
    return ms;
}
static std::vector<uint8_t> random_window(const Structure &ms, int n, int rate, int alphabet)
{
    std::vector<uint8_t> y;
    if (rnd_in(0, 5) == 0) { for (int i = 0; i < n; i++) y.push_back((uint8_t)rnd_in(0, alphabet - 1)); return y; }
    for (size_t s = 0; s < ms.size() && (int)y.size() < n + 8; s++)
        for (int k = rnd_in(0, 1 + n / (int)(ms[s].size() * ms.size())); k > 0; k--)
            for (uint8_t b : ms[s]) {
                const int e = rnd_in(0, 99) < rate ? rnd_in(0, 2) : 3;
                if (e == 0) y.push_back((uint8_t)rnd_in(0, alphabet - 1));
                else if (e == 1) { y.push_back(b); y.push_back((uint8_t)rnd_in(0, alphabet - 1)); }
                else if (e == 3) y.push_back(b);
            }
    while ((int)y.size() < n) y.push_back((uint8_t)rnd_in(0, alphabet - 1));
    y.resize((size_t)n);
    return y;
}

static int time_mode(const char *path)
{
    FILE *f = fopen(path, "rb");
    int32_t head[3] = { 0, 0, 0 };
    if (!f || fread(head, 4, 3, f) != 3 || head[0] < 0 || head[1] < 1 || head[1] > WS_MAX_WINDOW) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    const int N = head[0], len = head[1], kind = head[2];
    const Structure ms = kind == 0 ? Structure{ { 1, 0, 2 } } : Structure{ { 1, 0, 2 }, { 1, 0, 0 }, { 1, 1, 2, 1, 1, 0 }, { 1, 1, 2 } };
    const WsStruct st = pack(ms);
    std::vector<uint8_t> all((size_t)N * (size_t)len + 16);                                              // 8 bytes either side: the aligned word of the first and of the last base
    if (fread(all.data() + 8, 1, (size_t)N * (size_t)len, f) != (size_t)N * (size_t)len) { fprintf(stderr, "%s is short\n", path); return 2; }
    fclose(f);
    const int UB = kind == 0 ? 8 : 16, NW = we_row_words(UB);
    std::vector<uint32_t> rows((size_t)(len + 1) * (size_t)NW);
    std::vector<int32_t> list;
    long sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int w = 0; w < N; w++) {
        const uint8_t *at = all.data() + 8 + (size_t)w * (size_t)len;
        const int r = (int)((uintptr_t)at & 7);
        const auto ld = [at, r](int k) { uint64_t v; memcpy(&v, at - r + 8 * k, 8); return v; };
        uint32_t *rp = rows.data();
        const auto sink = [rp, NW, UB](int i, const WeRow &rec) { for (int k = 0; k < NW; k++) rp[(size_t)i * NW + k] = we_pack(UB, rec, k); };
        int end_id = 0;
        if (kind == 0) we_rows<8, false>(ld, sink, r, len, st, 1, 1, 1, end_id); else we_rows<16, true>(ld, sink, r, len, st, 1, 1, 1, end_id);
        const auto row = [rp, NW, UB](int i) { const uint32_t *p = rp + (size_t)i * NW; return we_unpack(UB, p[0], NW > 1 ? p[1] : 0u, 0u); };
        const auto base = [at](int p) { return at[p]; };
        const WeCount c = we_walk<false>(row, base, len, st, end_id, 0ull, 0, nullptr);
        list.resize((size_t)(c.edits + 1) * WE_FIELDS);
        const WeCount e = we_walk<true>(row, base, len, st, end_id, c.copies, c.edits, list.data() + (size_t)c.edits * WE_FIELDS);
        sum += e.edits;
    }
    const double ms_taken = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"windows\": %d, \"bases\": %d, \"structure\": %d, \"host_ms\": %.3f, \"edit_sum\": %ld}\n", N, len, kind, ms_taken, sum);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "--time")) return time_mode(argv[2]);
    const long cases = argc > 1 ? atol(argv[1]) : 12000;
    long runs = 0, edits = 0, kinds[3] = { 0, 0, 0 }, ups_on_last = 0, wrap_lefts = 0, row0_lefts = 0, start_ends = 0, skipped_segments = 0;
    for (long t = 0; t < cases; t++) {
        const bool wide = t % 3 == 2;
        const int W = wide ? W_WIDE[(t / 3) % 7] : W_NARROW[(t / 3) % 10];
        const int S = wide ? rnd_in(3, W < 4 ? 3 : 4) : rnd_in(1, W < 2 ? 1 : 2);
        const int *sc = SCORES[(t / 7) % 6];
        const int alphabet = rnd_in(1, 4), r = (int)(t % 8);
        const Structure ms = random_structure(S, W, alphabet);
        const int U0 = (int)ms[0].size();
        const int pick = (int)((t / 5) % 7);
        const int n = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? U0 - 1 : pick == 3 ? N_EDGES[(t / 35) % 9] : rnd_in(2, W <= 8 ? 40 : 70);
        const std::vector<uint8_t> y = random_window(ms, n, (int)((t / 11) % 3) * 12, alphabet);
        uint8_t *buf = (uint8_t *)malloc((size_t)(n > 0 ? n : 1));
        if (n > 0) memcpy(buf, y.data(), (size_t)n);
        const Brute want = brute(ms, buf, n, sc[0], sc[1], sc[2]);
        const WsStruct st = pack(ms);
        for (const auto &in : INST) {
            if (in.ub < W || (!in.wide && S > 2) || n == 0) continue;
            const Window w = { buf, n, r };
            const Got g = in.fn(w, st, sc[0], sc[1], sc[2]);
            const WsRaw walked = { g.raw.score, 0u, g.count.entry, g.count.copies, g.count.matches };
            int32_t seg[16];
            ws_spans(walked, n, S, seg);
            runs++;
            const char *why = nullptr;
            if (memcmp(&g.raw, &g.plain, sizeof(WsRaw))) why = "we_rows and ws_rows differ";
            else if (g.count.bad || g.emit.bad) why = "a walk gave up";
            else if (g.count.entry != g.raw.entry || g.count.copies != g.raw.copies || g.count.matches != g.raw.matches) why = "the walk's carried fields are not the rows'";
            else if (g.emit.edits != g.count.edits || g.emit.copies != g.count.copies) why = "the two walks differ";
            else if (g.raw.score != want.score || memcmp(seg, want.seg, sizeof seg)) why = "score or seg";
            else if (g.edits != want.edits) why = "the edits";
            for (int s = 0; s < S && !why; s++) {
                long k[3] = { 0, 0, 0 };
                for (size_t q = 0; q < g.edits.size(); q += WE_FIELDS) if (g.edits[q + 1] == s) k[g.edits[q + 4]]++;
                if (seg[4 * s + 2] * (long)ms[(size_t)s].size() != seg[4 * s + 3] + k[0] + k[2] || seg[4 * s + 1] - seg[4 * s] != seg[4 * s + 3] + k[0] + k[1]) why = "an invariant";
            }
            if (why) {
                fprintf(stderr, "FAIL (%s): case %ld %s scores (%d, %d, %d) residue %d: %s\n  header: score %d end %d edits%s\n  brute:  score %d edits%s\n", why, t, in.name, sc[0], sc[1], sc[2], r,
                        show(ms, buf, n).c_str(), g.raw.score, g.end_id, rows_of(g.edits).c_str(), want.score, rows_of(want.edits).c_str());
                return 1;
            }
        }
        if (n == 0 && (want.score != 0 || !want.edits.empty())) { fprintf(stderr, "FAIL: the brute force of an empty window is not zeros\n"); return 1; }
        edits += (long)want.edits.size() / WE_FIELDS;
        for (size_t q = 0; q < want.edits.size(); q += WE_FIELDS) kinds[want.edits[q + 4]]++;
        ups_on_last += want.ups_on_last; wrap_lefts += want.wrap_lefts; row0_lefts += want.row0_lefts;
        bool any = false;
        for (int s = 0; s < S; s++) { if (want.seg[4 * s + 2] == 0) skipped_segments++; else any = true; }
        if (!any && n > 0) start_ends++;
        free(buf);
    }
    if (runs < 10000 || !kinds[0] || !kinds[1] || !kinds[2] || !ups_on_last || !wrap_lefts || !row0_lefts || !start_ends || !skipped_segments) {
        fprintf(stderr, "FAIL: the cases are degenerate: %ld runs, kinds %ld %ld %ld, %ld ups on a last column, %ld wrap lefts, %ld lefts in row 0, %ld START ends, %ld skipped segments\n",
                runs, kinds[0], kinds[1], kinds[2], ups_on_last, wrap_lefts, row0_lefts, start_ends, skipped_segments);
        return 1;
    }
    printf("ok: %ld cases, %ld runs of we_rows and we_walk, %ld edits (%ld substitutions, %ld insertions, %ld deletions), %ld wrap lefts\n", cases, runs, edits, kinds[0], kinds[1], kinds[2], wrap_lefts);
    return 0;
}
