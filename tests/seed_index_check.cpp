// seed_index_check.cpp — the seed index of the catalogue genotype (mtr_amd/csrc/seed_index.h) for the host: a program of its own (the form a
// sanitizer build runs) that compares the window codes, the filter and the probe with brute force written here.  Every q of 8..16; windows at
// every residue of a 16-base word, the last window of a read, a read shorter than q (no window at all); the packed text holds exactly the words
// of the read, so a window that loads beyond them trips the address sanitizer; tables with duplicate codes (one run of several entries), with
// every code of a read planted and with none, a table filled to exactly half, and an empty table (cap = 0).
#include "../mtr_amd/csrc/seed_index.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

typedef std::vector<uint8_t> Seq;

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }      // xorshift32: every bit has the full period
static Seq rnd_seq(int n) { Seq s((size_t)n); for (auto &v : s) v = (uint8_t)(rnd() & 3u); return s; }

static long g_cases = 0;
static void fail(const char *what, long a, long b, long c)
{
    printf("FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
    exit(1);
}

// the device layout, sized to the read: ceil(L / 16) words and not one more
static std::vector<uint32_t> pack(const Seq &x)
{
    std::vector<uint32_t> w((x.size() + 15) / 16, 0u);
    for (size_t p = 0; p < x.size(); p++) w[p >> 4] |= (uint32_t)x[p] << (30 - 2 * (p & 15));
    return w;
}
struct Load { const uint32_t *w; uint32_t operator()(int k) const { return w[k]; } };

static uint32_t brute_code(const Seq &x, int pos, int q)
{
    uint64_t c = 0;
    for (int t = 0; t < q; t++) c = c * 4 + x[(size_t)(pos + t)];
    return (uint32_t)c;
}

struct Index {
    std::vector<uint32_t> filter, key; std::vector<int32_t> run, ent; int fbits; uint32_t cap;
    SiTable table() const { const SiTable t = { filter.data(), fbits, key.data(), run.data(), cap }; return t; }
};
// entries (code, value) -> the index as the library's host code makes it, in a table of cap slots
static Index build(std::vector<std::pair<uint32_t, int32_t>> e, int fbits, uint32_t cap)
{
    Index ix;
    ix.fbits = fbits; ix.cap = cap;
    ix.filter.assign(((size_t)1 << fbits) / 32, 0u); ix.key.assign(cap, 0u); ix.run.assign(2 * (size_t)cap, 0);
    std::sort(e.begin(), e.end());
    for (size_t k = 0, first = 0; k < e.size(); k++) {
        ix.ent.push_back(e[k].second);
        if (k + 1 < e.size() && e[k + 1].first == e[k].first) continue;
        si_filter_set(ix.filter.data(), fbits, e[k].first);
        if (!si_insert(ix.key.data(), ix.run.data(), cap, e[k].first, (int32_t)first, (int32_t)(k + 1 - first))) fail("the table is full", (long)k, cap, 0);
        first = k + 1;
    }
    return ix;
}

static void check_codes(int q, int L)
{
    const Seq x = rnd_seq(L);
    const std::vector<uint32_t> w = pack(x);
    const Load ld = { w.data() };
    for (int pos = 0; pos + q <= L; pos++) {          // (a read shorter than q has no window: nothing is loaded)
        const uint32_t got = si_window_code(ld, pos, q), want = brute_code(x, pos, q);
        if (got != want) fail("window code", q, L, pos);
        if (si_seed_code(x.data() + pos, q) != want) fail("seed code", q, L, pos);
        g_cases++;
    }
}

static void check_table(int q, int L, int planted_every, int dup, bool half_full)
{
    const Seq x = rnd_seq(L);
    const std::vector<uint32_t> w = pack(x);
    const Load ld = { w.data() };
    std::vector<std::pair<uint32_t, int32_t>> e;
    std::map<uint32_t, std::vector<int32_t>> want;
    int32_t v = 0;
    for (int pos = 0; planted_every > 0 && pos + q <= L; pos += planted_every)
        for (int d = 0; d < dup; d++) { e.push_back({ brute_code(x, pos, q), v }); want[brute_code(x, pos, q)].push_back(v); v++; }
    for (int k = 0; k < 40; k++) { const Seq s = rnd_seq(q); e.push_back({ si_seed_code(s.data(), q), v }); want[si_seed_code(s.data(), q)].push_back(v); v++; }
    uint32_t cap = 64;
    while (cap < 2 * want.size()) cap <<= 1;
    if (half_full) while (want.size() < cap / 2) { const Seq s = rnd_seq(q); const uint32_t c = si_seed_code(s.data(), q); if (!want.count(c)) { e.push_back({ c, v }); want[c].push_back(v); v++; } }
    const Index ix = build(e, 15, cap);
    const SiTable t = ix.table();
    for (int pos = 0; pos + q <= L; pos++) {
        const uint32_t code = si_window_code(ld, pos, q);
        const auto it = want.find(code);
        const SiRun r = si_probe(t, code);
        if (it == want.end()) { if (r.count != 0) fail("a run for no seed", q, pos, r.count); }
        else {
            if (!si_filter_has(t, code)) fail("the filter drops a seed", q, pos, 0);
            if (r.count != (int32_t)it->second.size()) fail("run length", q, pos, r.count);
            std::vector<int32_t> got(ix.ent.begin() + r.first, ix.ent.begin() + r.first + r.count);
            std::sort(got.begin(), got.end());
            if (got != it->second) fail("run entries", q, pos, r.first);
        }
        g_cases++;
    }
    for (const auto &kv : want) {
        if (!si_filter_has(t, kv.first) || si_probe(t, kv.first).count != (int32_t)kv.second.size()) fail("a planted seed is lost", q, (long)kv.first, 0);
        g_cases++;
    }
}

int main()
{
    for (int q = SI_MIN_Q; q <= SI_MAX_Q; q++) {
        for (int L : { 0, 1, q - 1, q, q + 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 257 }) check_codes(q, L);      // every residue of a word, the last window on every residue
        for (int L = 60; L < 76; L++) check_codes(q, L);
        check_table(q, 300, 0, 1, false);           // nothing of the read planted
        check_table(q, 300, 7, 1, false);
        check_table(q, 300, 1, 1, false);           // every window a seed
        check_table(q, 200, 5, 3, false);           // duplicate codes: runs of three entries
        check_table(q, 200, 3, 2, true);            // the table filled to exactly half
        check_table(q, q - 1, 1, 1, false);         // a read shorter than q
        // the empty table: no seed at all
        const uint32_t none = 0;
        const SiTable empty = { &none, 5, nullptr, nullptr, 0 };
        const Seq s = rnd_seq(q);
        if (si_filter_has(empty, si_seed_code(s.data(), q)) || si_probe(empty, si_seed_code(s.data(), q)).count != 0) fail("the empty table", q, 0, 0);
        if (si_seed_offset(3, q) != 3 * q) fail("seed offset", q, 0, 0);
        g_cases++;
    }
    printf("%ld cases checked: ok\n", g_cases);
    return 0;
}
