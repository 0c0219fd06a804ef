// motif_dp_check.cpp — the per-lane DP of the known-motif search (mtr_amd/csrc/motif_dp.h) for the host: a program of its own (the form a
// sanitizer build runs) that compares all nine outputs of motif_dp<UB>() with a naive full-matrix DP written here from the definition of
// include/mtr_hip.h.  Every bucket runs at its smallest and largest U; reads are random, noisy tandems that start mid-unit, two equal runs
// and reads without a hit; lengths include 1 and lengths around the motif's; and groups of 64 "lanes" of unequal length share ONE interleaved
// cell buffer of exactly the size the kernel's host side gives a wavefront - all forward passes first, then all tracebacks, so a lane that
// leaves its slice either trips the address sanitizer or corrupts a neighbour's path.
#include "../mtr_amd/csrc/motif_dp.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

// the definition: the whole matrix, the reference's loops
static MotifHit naive(const std::vector<uint8_t> &x, const std::vector<uint8_t> &m, int G, int MM, int D)
{
    const int L = (int)x.size(), U = (int)m.size(), nx = U + 1;
    std::vector<int> H((size_t)(L + 1) * (size_t)nx, 0);
    int best = 0, bi = 0, bj = 0;
    for (int i = 1; i <= L; i++) {
        for (int j = 1; j <= U; j++) {
            const int diag = H[(size_t)(i - 1) * nx + j - 1], up = H[(size_t)(i - 1) * nx + j];
            int v;
            if (x[(size_t)i - 1] == m[(size_t)j - 1]) v = diag + G;
            else {
                v = std::max(0, std::max(diag - MM, up - D));
                if (j > 1) v = std::max(v, H[(size_t)i * nx + j - 1] - D);
            }
            H[(size_t)i * nx + j] = v;
            if (v > best) { best = v; bi = i; bj = j; }
        }
        H[(size_t)i * nx] = H[(size_t)i * nx + U];
    }
    MotifHit r = { 0, -1, 0, 0, 0, 0, 0, 0, 0 };
    if (best <= 0) return r;
    int i = bi, j = bj, cur = best, mat = 0, mis = 0, ins = 0, del = 0;
    while (i > 0 && H[(size_t)i * nx + j] > 0) {
        const int diag = H[(size_t)(i - 1) * nx + j - 1], up = H[(size_t)(i - 1) * nx + j], left = H[(size_t)i * nx + j - 1];
        const bool eq = x[(size_t)i - 1] == m[(size_t)j - 1];
        if (cur == diag + G && eq) { cur -= G; i--; j--; mat++; }
        else if (cur == diag - MM && !eq) { cur += MM; i--; j--; mis++; }
        else if (cur == left - D) { cur += D; j--; del++; }
        else if (cur == up - D) { cur += D; i--; ins++; }
        else break;
        if (j == 0) j = U;
    }
    r.start = i; r.end = bi - 1; r.repeat_len = bi - i; r.copies = (mat + mis + del) / U;
    r.mat = mat; r.mis = mis; r.ins = ins; r.del = del; r.score = best;
    return r;
}

static std::vector<uint32_t> pack(const std::vector<uint8_t> &x)
{
    std::vector<uint32_t> w((x.size() + 15) / 16, 0u);            // exactly the words the read touches: a load past them is the sanitizer's
    for (size_t i = 0; i < x.size(); i++) w[i >> 4] |= (uint32_t)(x[i] & 3) << (30 - 2 * (i & 15));
    return w;
}

static uint32_t g_x = 2463534242u;
static uint32_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 17; g_x ^= g_x << 5; return g_x; }

enum { RANDOM = 0, TANDEM, TWO_RUNS, NO_HIT, N_KINDS };
static std::vector<uint8_t> make_read(int kind, int L, const std::vector<uint8_t> &m)
{
    const int U = (int)m.size();
    std::vector<uint8_t> x((size_t)L);
    if (kind == RANDOM) for (auto &c : x) c = (uint8_t)(rnd() & 3);
    if (kind == TANDEM) {                                           // starts mid-unit; one base in eleven is changed, dropped or doubled
        size_t n = 0; int ph = U / 2;
        while (n < x.size()) {
            const uint32_t e = rnd() % 33;
            if (e == 0) { x[n++] = (uint8_t)((m[(size_t)(ph % U)] + 1 + rnd() % 3) & 3); ph++; }
            else if (e == 1) ph++;
            else if (e == 2) x[n++] = (uint8_t)(rnd() & 3);
            else { x[n++] = m[(size_t)(ph % U)]; ph++; }
        }
    }
    if (kind == TWO_RUNS) {                                         // run, junk, the same run again: the first must win
        const int run = std::max(1, L / 3);
        for (int i = 0; i < L; i++) x[(size_t)i] = m[(size_t)(i % U)];
        bool in[4] = { false, false, false, false };
        for (uint8_t c : m) in[c] = true;
        int out = -1;
        for (int c = 0; c < 4; c++) if (!in[c]) out = c;
        for (int i = run; i < L - run; i++) x[(size_t)i] = out >= 0 ? (uint8_t)out : (uint8_t)((m[(size_t)(i % U)] + 2) & 3);
        for (int i = std::max(run, L - run); i < L; i++) x[(size_t)i] = m[(size_t)((i - (L - run)) % U)];
    }
    if (kind == NO_HIT) {                                           // a base the motif does not hold, where there is one
        bool in[4] = { false, false, false, false };
        for (uint8_t c : m) in[c] = true;
        int out = 0;
        for (int c = 0; c < 4; c++) if (!in[c]) out = c;
        for (auto &c : x) c = (uint8_t)out;
    }
    return x;
}

template <int UB>
static MotifHit run_bucket(const uint32_t *pk, int L, uint64_t mot, int U, int G, int MM, int D, const MdpCellsLane &c, bool forward_only, int *best)
{
    if (forward_only) { motif_dp_forward<UB>(pk, L, mot, U, G, MM, D, c, best[0], best[1], best[2]); return MotifHit{}; }
    return motif_dp_traceback(c, U, best[0], best[1], best[2]);
}
static MotifHit run(const uint32_t *pk, int L, uint64_t mot, int U, int G, int MM, int D, const MdpCellsLane &c, bool forward_only, int *best)
{
    switch (mdp_bucket(U)) {
    case 4: return run_bucket<4>(pk, L, mot, U, G, MM, D, c, forward_only, best);
    case 8: return run_bucket<8>(pk, L, mot, U, G, MM, D, c, forward_only, best);
    case 16: return run_bucket<16>(pk, L, mot, U, G, MM, D, c, forward_only, best);
    default: return run_bucket<32>(pk, L, mot, U, G, MM, D, c, forward_only, best);
    }
}

static long g_checked = 0, g_hits = 0;
static bool same(const MotifHit &a, const MotifHit &b) { return memcmp(&a, &b, sizeof a) == 0; }

// 64 lanes, lane l with read reads[l] (an empty read: a lane without a task), one buffer
static bool check_group(const std::vector<std::vector<uint8_t>> &reads, const std::vector<uint8_t> &m, int G, int MM, int D)
{
    const int U = (int)m.size(), nd = mdp_dwords(U);
    size_t rows = 0;
    for (const auto &x : reads) rows = std::max(rows, x.size());
    std::vector<uint32_t> cells(rows * (size_t)nd * 64, 0xeeeeeeeeu);
    const uint64_t mot = mdp_motif_bits(m.data(), U);
    std::vector<std::vector<uint32_t>> pk;
    for (const auto &x : reads) pk.push_back(pack(x));
    int best[64][3];
    for (int l = 0; l < 64; l++) {
        const MdpCellsLane c = { cells.data(), nd, l };
        (void)run(pk[(size_t)l].data(), (int)reads[(size_t)l].size(), mot, U, G, MM, D, c, true, best[l]);
    }
    bool ok = true;
    for (int l = 0; l < 64; l++) {
        const MdpCellsLane c = { cells.data(), nd, l };
        const MotifHit got = run(nullptr, 0, mot, U, G, MM, D, c, false, best[l]), want = naive(reads[(size_t)l], m, G, MM, D);
        if (!reads[(size_t)l].empty()) { g_checked++; g_hits += want.score > 0; }
        const bool identity = got.score == G * got.mat - MM * got.mis - D * (got.ins + got.del);
        if (!same(got, want) || !identity) {
            fprintf(stderr, "U %d L %zu scores %d %d %d lane %d: got (%d %d %d %d %d %d %d %d %d), want (%d %d %d %d %d %d %d %d %d)\n", U, reads[(size_t)l].size(), G, MM, D, l,
                    got.start, got.end, got.repeat_len, got.copies, got.mat, got.mis, got.ins, got.del, got.score,
                    want.start, want.end, want.repeat_len, want.copies, want.mat, want.mis, want.ins, want.del, want.score);
            ok = false;
        }
    }
    return ok;
}

int main()
{
    static const int scores[4][3] = { { 5, 1, 1 }, { 1, 1, 3 }, { 1, 3, 1 }, { 1, 1, 1 } };
    bool ok = true;
    for (int U : { 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32 }) {             // every bucket's smallest and largest U, and lengths that end inside a dword
        for (int alphabet : { 4, 2 }) {
            std::vector<uint8_t> m((size_t)U);
            for (auto &c : m) c = (uint8_t)(rnd() % (uint32_t)alphabet);
            for (const auto &s : scores) {
                // single lanes at the lengths where something changes
                for (int L : { 1, 2, 3, U, U + 1, 15, 16, 17, 40, 97 })
                    for (int kind = 0; kind < N_KINDS; kind++) {
                        std::vector<std::vector<uint8_t>> reads(64);
                        reads[(size_t)(rnd() & 63)] = make_read(kind, L, m);
                        ok = check_group(reads, m, s[0], s[1], s[2]) && ok;
                    }
                // a full group of unequal lengths, longest first as the search orders them, and one in any order with lanes left out
                std::vector<std::vector<uint8_t>> sorted(64), mixed(64);
                for (int l = 0; l < 64; l++) {
                    sorted[(size_t)l] = make_read(l % N_KINDS, 130 - 2 * l, m);
                    if (l % 7 != 3) mixed[(size_t)l] = make_read((l / 3) % N_KINDS, 1 + (int)(rnd() % 120), m);
                }
                ok = check_group(sorted, m, s[0], s[1], s[2]) && ok;
                ok = check_group(mixed, m, s[0], s[1], s[2]) && ok;
            }
        }
    }
    printf("%ld alignments checked (%ld with a hit): %s\n", g_checked, g_hits, ok ? "ok" : "FAILED");
    return ok && g_hits > g_checked / 4 ? 0 : 1;
}
