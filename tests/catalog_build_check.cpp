// catalog_build_check.cpp — what the device build of a prepared catalogue shares with the host (mtr_amd/csrc/catalog_build.h), as a program of its
// own (the form a sanitizer build runs), against brute force written here: a slot's codes and the reverse complement for every flank length
// 1..64 (the buffers hold exactly the pattern, so a byte beyond it trips the address sanitizer), a motif's two strands and the reversed 2-bit
// form, the digits of a code for every seed length, and the sort as the kernels run it - a wavefront of 64 lanes a step, tiles of CB_TILE
// entries, per tile the digits' counts, their exclusive sums over (digit, tile), an entry placed by what the earlier steps counted plus its
// rank among its peers (cb_peers / cb_peer_rank / cb_peer_last over emulated ballots) - against std::stable_sort, for totals either side of
// a wavefront, of 256 and of a tile; then the duplicate drop and the run heads against std::unique, and the table's sizes against their rule.
#include "../mtr_amd/csrc/catalog_build.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }      // xorshift32

static long g_cases = 0;
static void fail(const char *what, long a, long b, long c)
{
    printf("FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
    exit(1);
}

static std::string rnd_letters(int n) { std::string s((size_t)n, 'A'); for (auto &c : s) c = "ACGT"[rnd() & 3u]; return s; }
static int brute_code(char c) { for (int k = 0; k < 4; k++) if (c == "ACGT"[k]) return k; return -1; }

static void check_codes()
{
    for (int c = 0; c < 256; c++) { if (cb_base_code((char)c) != brute_code((char)c)) fail("base code", c, 0, 0); g_cases++; }
    for (int m = 1; m <= CB_MAX_M; m++)
        for (int rep = 0; rep < 8; rep++) {
            const std::string f = rnd_letters(m);
            const std::vector<char> exact(f.begin(), f.end());                      // exactly m bytes: no terminator to read by mistake
            for (int j = 0; j < 4; j++) {
                std::vector<uint8_t> got((size_t)m);
                cb_slot_codes(exact.data(), m, j, got.data());
                for (int t = 0; t < m; t++) {
                    const int want = j < 2 ? brute_code(f[(size_t)t]) : 3 - brute_code(f[(size_t)(m - 1 - t)]);
                    if (got[(size_t)t] != want) fail("slot codes", m, j, t);
                }
                g_cases++;
            }
        }
    for (int U : { 1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 64, 499 })
        for (int rep = 0; rep < 8; rep++) {
            const std::string f = rnd_letters(U);
            const std::vector<char> exact(f.begin(), f.end());
            std::vector<uint8_t> fwd((size_t)U), rc((size_t)U);
            cb_motif_codes(exact.data(), U, 0, fwd.data()); cb_motif_codes(exact.data(), U, 1, rc.data());
            for (int t = 0; t < U; t++)
                if (fwd[(size_t)t] != brute_code(f[(size_t)t]) || rc[(size_t)t] != 3 - brute_code(f[(size_t)(U - 1 - t)])) fail("motif codes", U, t, 0);
            if (U <= 32) {
                uint64_t bits = 0, want = 0;
                for (int j = 0; j < U; j++) { bits |= (uint64_t)fwd[(size_t)j] << (2 * j); want |= (uint64_t)fwd[(size_t)(U - 1 - j)] << (2 * j); }
                if (cb_bits_reversed(bits, U) != want) fail("reversed bits", U, 0, 0);
                if (cb_bits_reversed(cb_bits_reversed(bits, U), U) != bits) fail("reversed twice", U, 0, 0);
            }
            g_cases++;
        }
}

static void check_digits()
{
    for (int q = 8; q <= 16; q++) {
        const int passes = cb_passes(q);
        if (passes != (q <= 8 ? 2 : q <= 12 ? 3 : 4)) fail("passes", q, passes, 0);
        for (int rep = 0; rep < 200; rep++) {
            const uint32_t key = q == 16 ? (rnd() << 4) ^ rnd() : ((rnd() << 4) ^ rnd()) & ((1u << (2 * q)) - 1);
            uint32_t back = 0;
            for (int p = 0; p < passes; p++) {
                const uint32_t d = cb_digit(key, p);
                if (d >= CB_DIGITS) fail("digit range", q, p, (long)d);
                back |= d << (CB_DIGIT_BITS * p);
            }
            if (back != key) fail("digits do not make the key", q, (long)key, (long)back);
            g_cases++;
        }
    }
    if (cb_popc64(0) != 0 || cb_popc64(~(uint64_t)0) != 64 || cb_popc64(0x8000000000000001ull) != 2) fail("popc", 0, 0, 0);
}

typedef std::pair<uint32_t, int32_t> Ent;

// a wavefront's step: the ballots of the 64 lanes' digit bits, then every lane's peers
struct Step { bool has[64]; uint32_t digit[64]; uint64_t peers[64]; };
static Step step_of(const std::vector<Ent> &in, size_t e0, int pass)
{
    Step s;
    uint64_t ballot[CB_DIGIT_BITS] = { 0 }, active = 0;
    for (int lane = 0; lane < 64; lane++) {
        const size_t e = e0 + (size_t)lane;
        s.has[lane] = e < in.size();
        s.digit[lane] = cb_digit(s.has[lane] ? in[e].first : 0u, pass);
        if (!s.has[lane]) continue;
        active |= (uint64_t)1 << lane;
        for (int b = 0; b < CB_DIGIT_BITS; b++) if ((s.digit[lane] >> b) & 1) ballot[b] |= (uint64_t)1 << lane;
    }
    for (int lane = 0; lane < 64; lane++) {
        s.peers[lane] = cb_peers(ballot, s.digit[lane], active);
        if (!s.has[lane]) continue;
        uint64_t want = 0;                                   // brute force: the lanes with an entry of this digit
        for (int o = 0; o < 64; o++) if (s.has[o] && s.digit[o] == s.digit[lane]) want |= (uint64_t)1 << o;
        if (s.peers[lane] != want) fail("peers", lane, (long)s.digit[lane], 0);
        int lower = 0; bool higher = false;
        for (int o = 0; o < 64; o++) if ((want >> o) & 1) { lower += o < lane; higher = higher || o > lane; }
        if (cb_peer_rank(s.peers[lane], lane) != lower || cb_peer_last(s.peers[lane], lane) != !higher) fail("peer rank", lane, lower, higher);
    }
    return s;
}

// one pass as mtr_k_catb_count, the scan, and mtr_k_catb_fill run it
static std::vector<Ent> radix_pass(const std::vector<Ent> &in, int pass)
{
    const size_t n = in.size(), tiles = (n + CB_TILE - 1) / CB_TILE;
    std::vector<uint32_t> hist((size_t)CB_DIGITS * tiles, 0u);
    for (size_t tile = 0; tile < tiles; tile++)
        for (int st = 0; st < CB_TILE / 64; st++) {
            const Step s = step_of(in, tile * CB_TILE + (size_t)st * 64, pass);
            for (int lane = 0; lane < 64; lane++)
                if (s.has[lane] && cb_peer_last(s.peers[lane], lane)) hist[(size_t)s.digit[lane] * tiles + tile] += (uint32_t)cb_popc64(s.peers[lane]);
        }
    std::vector<uint64_t> first(hist.size() + 1, 0);
    for (size_t k = 0; k < hist.size(); k++) first[k + 1] = first[k] + hist[k];
    if (first[hist.size()] != n) fail("the counts do not add up", (long)n, (long)first[hist.size()], pass);
    std::vector<Ent> out(n);
    std::vector<bool> written(n, false);
    for (size_t tile = 0; tile < tiles; tile++) {
        uint32_t at[CB_DIGITS];
        for (int d = 0; d < CB_DIGITS; d++) at[d] = (uint32_t)first[(size_t)d * tiles + tile];
        for (int st = 0; st < CB_TILE / 64; st++) {
            const size_t e0 = tile * CB_TILE + (size_t)st * 64;
            const Step s = step_of(in, e0, pass);
            size_t pos[64];
            for (int lane = 0; lane < 64; lane++) pos[lane] = (size_t)at[s.digit[lane]] + (size_t)cb_peer_rank(s.peers[lane], lane);
            for (int lane = 0; lane < 64; lane++) if (s.has[lane] && cb_peer_last(s.peers[lane], lane)) at[s.digit[lane]] += (uint32_t)cb_popc64(s.peers[lane]);
            for (int lane = 0; lane < 64; lane++) {
                if (!s.has[lane]) continue;
                if (pos[lane] >= n || written[pos[lane]]) fail("a place out of range or taken twice", (long)pos[lane], (long)n, pass);
                out[pos[lane]] = in[e0 + (size_t)lane]; written[pos[lane]] = true;
            }
        }
    }
    return out;
}

static void check_sort()
{
    const size_t totals[] = { 1, 2, 63, 64, 65, 255, 256, 257, CB_TILE - 1, CB_TILE, CB_TILE + 1, 2 * CB_TILE + 77, 5000 };
    for (int q : { 8, 11, 12, 16 })
        for (size_t n : totals)
            for (int kind = 0; kind < 3; kind++) {
                // kind 0: random codes; 1: few codes, many entries each (runs longer than a wavefront and than 256); 2: codes 0 and all ones among them
                const uint32_t mask = q == 16 ? 0xFFFFFFFFu : (1u << (2 * q)) - 1;
                std::vector<Ent> ent(n);
                for (size_t e = 0; e < n; e++) {
                    uint32_t code = ((rnd() << 4) ^ rnd()) & mask;
                    if (kind == 1) code = (code % 3) * 0x01010101u & mask;
                    if (kind == 2 && rnd() % 4 == 0) code = rnd() & 1 ? mask : 0u;
                    ent[e] = { code, (int32_t)(e / 2) };                     // slots ascend, each twice: the emitting order, with duplicates to drop
                }
                std::vector<Ent> want = ent;
                std::stable_sort(want.begin(), want.end(), [](const Ent &a, const Ent &b) { return a.first < b.first; });
                std::vector<Ent> got = ent;
                for (int p = 0; p < cb_passes(q); p++) got = radix_pass(got, p);
                if (got != want) fail("the sort is not the stable sort", q, (long)n, kind);
                if (!std::is_sorted(got.begin(), got.end())) fail("stable by code does not leave (code, slot) sorted", q, (long)n, kind);
                // the duplicate drop and the heads
                std::vector<Ent> kept; size_t heads = 0;
                for (size_t e = 0; e < n; e++) {
                    const bool first = e == 0;
                    const Ent prev = first ? Ent(0u, 0) : got[e - 1];
                    if (cb_keep(first, got[e].first, got[e].second, prev.first, prev.second)) kept.push_back(got[e]);
                    const bool head = cb_head(first, got[e].first, prev.first);
                    if (head && !cb_keep(first, got[e].first, got[e].second, prev.first, prev.second)) fail("a head that is dropped", q, (long)n, (long)e);
                    heads += head;
                }
                std::vector<Ent> uniq = want;
                std::sort(uniq.begin(), uniq.end());
                uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
                if (kept != uniq) fail("the duplicate drop", q, (long)n, kind);
                size_t distinct = 0;
                for (size_t e = 0; e < uniq.size(); e++) distinct += e == 0 || uniq[e].first != uniq[e - 1].first;
                if (heads != distinct) fail("the heads", q, (long)heads, (long)distinct);
                g_cases++;
            }
}

static void check_sizes()
{
    for (uint64_t d : { 1ull, 2ull, 31ull, 32ull, 33ull, 2047ull, 2048ull, 2049ull, 65535ull, 65536ull, 65537ull, 1000000ull, 1048576ull, 1048577ull, 40000000ull }) {
        const uint32_t cap = cb_table_cap(d);
        if (cap < 64 || (cap & (cap - 1)) || cap < 2 * d || (cap > 64 && cap / 2 >= 2 * d)) fail("table slots", (long)d, (long)cap, 0);
        const int fbits = cb_filter_bits(d);
        if (fbits < CB_FILTER_MIN_BITS || fbits > CB_FILTER_MAX_BITS) fail("filter bits range", (long)d, fbits, 0);
        if (fbits < CB_FILTER_MAX_BITS && ((uint64_t)1 << fbits) < 16 * d) fail("filter too small", (long)d, fbits, 0);
        if (fbits > CB_FILTER_MIN_BITS && ((uint64_t)1 << (fbits - 1)) >= 16 * d) fail("filter too large", (long)d, fbits, 0);
        g_cases++;
    }
}

int main()
{
    check_codes();
    check_digits();
    check_sort();
    check_sizes();
    printf("%ld cases checked: ok\n", g_cases);
    return 0;
}
