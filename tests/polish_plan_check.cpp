// polish_plan_check.cpp — polish_repeat as the kernels run it (mtr_amd/csrc/polish_plan.h) for the host: built by the plain host C++ compiler
// into a small shared library and called from tests/test_polish_plan_host.py, which holds the plan to the CPU oracle's polish calls and to the
// reference's walk over every position compiled from the same header.  With -DPOLISH_PLAN_CHECK_MAIN it is a program of its own that runs
// the random comparison (the build under -fsanitize=address,undefined runs this way).
#include "../mtr_amd/csrc/walk_screen.h"
#include "../mtr_amd/csrc/polish_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace {
struct HostOps {                              // polish_plan.h's OPS over arrays and a map
    const uint8_t *u; const uint8_t *sc; int k, period;
    const std::unordered_map<int, int> *tab;
    uint8_t out[MTRC_MAX_PERIOD];
    int n_undefined = 0, n_lookups = 0, n_copied = 0, n_body = 0;
    int base(int j) const { return u[j] & 3; }
    int score(int j) const { return j < 0 ? 0 : sc[j]; }      // (before the unit's start: a low score, so that a predicate that looks there is caught and not undefined)
    int get(int node) { n_lookups++; auto it = tab->find(node); return it == tab->end() ? 0 : it->second; }
    void get4(int a0, int a1, int a2, int a3, int &f0, int &f1, int &f2, int &f3) { f0 = get(a0); f1 = get(a1); f2 = get(a2); f3 = get(a3); }
    int cyc(int j) { return pp_cyc(*this, k, period, j); }
    void emit(int jr, int b) { n_body++; out[jr] = (uint8_t)b; }
    void copy(int jr, int j, int n) { n_copied += n; for (int i = 0; i < n; i++) out[jr - i] = (uint8_t)base(j - i); }
    void undefined() { n_undefined++; }
    void join() {}
};

// the k-mer table of window [qs, qe] of a packed read: a plain map over win_node (init_inputString + counting, consensus.c:37-60, :138-196)
void window_table(std::unordered_map<int, int> &tab, const uint32_t *pk, int L, int k, int qs, int qe)
{
    for (int i = qs; i <= qe; i++) tab[win_node(pk, L, k, qe, i)]++;
}

// polish() of k2_units.hip.inc, step for step: returns the new period; out_unit = the polished unit (the input where nothing changes).
// info: [0] flagged positions, [1] int_unit[-1] reads, [2] 1 = the walk altered a position, [3] 1 = the output outgrew MTRC_MAX_PERIOD,
//       [4] table look-ups, [5] positions copied in stretches, [6] positions through the loop body, [7] 1 = the table was built
int polish_host(int walk_all, const uint32_t *pk, int L, int rs, int re, int k, int period, const uint8_t *unit, const int32_t *score,
                uint8_t *out_unit, int32_t *info)
{
    for (int i = 0; i < 8; i++) info[i] = 0;
    memcpy(out_unit, unit, (size_t)(period > 0 ? period : 0));
    if (period <= k) return period;
    std::vector<uint8_t> st((size_t)period), base((size_t)period), sc((size_t)period);
    for (int t = 0; t < period; t++) { st[t] = pp_stage_byte(unit[t], score[t]); base[t] = st[t] & 3; sc[t] = (st[t] >> 2) & 3; }
    PpMask m;
    pp_mask_build(m, [&](int t) { return t < 0 ? 0 : (int)sc[t]; }, k, period);
    for (int j = 0; j < period; j++) info[0] += pp_mask_test(m, j) ? 1 : 0;
    if (!pp_mask_any(m)) return period;
    std::unordered_map<int, int> tab;
    window_table(tab, pk, L, k, rs, re);
    info[7] = 1;
    HostOps ops{base.data(), sc.data(), k, period, &tab, {0}};
    int jr = 0; bool altered = false;
    const bool ok = walk_all ? pp_walk_all(ops, k, period, jr, altered) : pp_walk_plan(ops, m, k, period, jr, altered);
    info[1] = ops.n_undefined; info[2] = altered ? 1 : 0; info[3] = ok ? 0 : 1; info[4] = ops.n_lookups; info[5] = ops.n_copied; info[6] = ops.n_body;
    if (!ok) return period;
    const int np = (MTRC_MAX_PERIOD - 1) - jr;
    for (int t = 0; t < np; t++) out_unit[t] = ops.out[t + jr + 1];
    return np;
}

struct Rng { unsigned long long s; unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); } int below(int n) { return (int)(next() % (unsigned)n); } };
}

// walk_all = 0: the plan; 1: the reference's walk over every position.  pk: the read's bases 2 bits each, first base in the top bits of word 0, at
// least one zero word behind the last.  out_unit: MTRC_MAX_PERIOD bytes.  info: 8 ints (polish_host).
extern "C" int32_t pp_check_polish(int32_t walk_all, const uint32_t *pk, int32_t L, int32_t rep_start, int32_t rep_end, int32_t k, int32_t period,
                                   const uint8_t *unit, const int32_t *score, uint8_t *out_unit, int32_t *info)
{
    return polish_host(walk_all, pk, L, rep_start, rep_end, k, period, unit, score, out_unit, info);
}

// n random (unit, scores, k) triples, the plan against the walk over every position, call for call.  The window is the unit repeated with
// substitutions, insertions and deletions, so that the table offers alternatives; the scores come in runs of 0 / 1 long enough to be
// suspicious, so that about a tenth of the positions are flagged.  stats: [0] calls, [1] calls that differ (unit, length, or any count of info
// but the look-ups), [2] positions, [3] flagged positions, [4] calls with an altered position, [5] calls whose length changed, [6] calls whose
// output outgrew MTRC_MAX_PERIOD, [7] int_unit[-1] reads, [8] look-ups of the plan, [9] look-ups of the walk over every position.
extern "C" void pp_random_compare(int32_t n, uint64_t seed, int64_t *stats)
{
    Rng g{seed * 2654435761ull + 12345ull};
    for (int i = 0; i < 10; i++) stats[i] = 0;
    static const int ks[] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    for (int it = 0; it < n; it++) {
        const int k = ks[g.below(11)];
        int period;
        const int cls = g.below(10);
        if (cls == 0) period = 2 + g.below(12);                           // around k: period <= k among them
        else if (cls == 1) period = 480 + g.below(20);                    // near MTRC_MAX_PERIOD: an insertion or two overflows
        else if (cls == 2) period = 60 + g.below(10);                     // around a mask word's end
        else period = 6 + g.below(250);
        std::vector<uint8_t> unit((size_t)period);
        for (auto &b : unit) b = (uint8_t)g.below(4);
        // the window: copies of a variant of the unit, each copy with its own rare errors
        std::vector<uint8_t> var;
        for (int t = 0; t < period; t++) {
            const int e = g.below(40);
            if (e == 0) continue;                                         // the unit has a base the repeat lacks
            if (e == 1) var.push_back((uint8_t)g.below(4));               // the repeat has a base the unit lacks
            var.push_back(e == 2 ? (uint8_t)g.below(4) : unit[t]);
        }
        if (var.empty()) var.push_back(0);
        const int copies = 3 + g.below(6), lead = g.below(20);
        std::vector<uint8_t> read;
        for (int t = 0; t < lead; t++) read.push_back((uint8_t)g.below(4));
        const int rs = (int)read.size();
        for (int c = 0; c < copies; c++) for (uint8_t b : var) read.push_back(g.below(50) == 0 ? (uint8_t)g.below(4) : b);
        const int re = (int)read.size() - 1;
        const int tail = g.below(3) == 0 ? 0 : g.below(20);               // a third of the windows end with the read (raw-base nodes)
        for (int t = 0; t < tail; t++) read.push_back((uint8_t)g.below(4));
        const int L = (int)read.size();
        std::vector<uint32_t> pk((size_t)L / 16 + 3, 0u);
        for (int t = 0; t < L; t++) pk[t >> 4] |= (uint32_t)read[t] << (30 - 2 * (t & 15));
        std::vector<int32_t> score((size_t)period);
        for (int t = 0; t < period;) {
            if (g.below(19) == 0) { const int run = 1 + g.below(2 * k + 2); for (int q = 0; q < run && t < period; q++, t++) score[t] = g.below(5) == 0 ? 0 : (g.below(12) == 0 ? 2 : 1); }
            else { score[t] = g.below(20) == 0 ? -1 : 2 + g.below(6); t++; }
        }
        uint8_t o0[MTRC_MAX_PERIOD], o1[MTRC_MAX_PERIOD]; int32_t i0[8], i1[8];
        const int p0 = polish_host(0, pk.data(), L, rs, re, k, period, unit.data(), score.data(), o0, i0);
        const int p1 = polish_host(1, pk.data(), L, rs, re, k, period, unit.data(), score.data(), o1, i1);
        bool same = p0 == p1 && memcmp(o0, o1, (size_t)(p0 > 0 ? p0 : 0)) == 0;
        for (int q = 0; q < 4; q++) same = same && i0[q] == i1[q];
        same = same && i0[7] == i1[7] && (i1[3] != 0 || i0[5] + i0[6] == i1[6]);        // (an overflow ends the plan inside a stretch: fewer emissions)
        stats[0]++; if (!same) stats[1]++;
        stats[2] += period; stats[3] += i0[0]; stats[4] += i1[2]; if (p1 != period) stats[5]++; stats[6] += i1[3]; stats[7] += i1[1];
        stats[8] += i0[4]; stats[9] += i1[4];
    }
}

#ifdef POLISH_PLAN_CHECK_MAIN
int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 20000;
    int64_t s[10];
    pp_random_compare(n, argc > 2 ? (uint64_t)atoll(argv[2]) : 1ull, s);
    printf("calls %lld differ %lld positions %lld flagged %lld altered %lld length_changed %lld overflowed %lld undefined %lld lookups_plan %lld lookups_all %lld\n",
           (long long)s[0], (long long)s[1], (long long)s[2], (long long)s[3], (long long)s[4], (long long)s[5], (long long)s[6], (long long)s[7],
           (long long)s[8], (long long)s[9]);
    return s[1] == 0 ? 0 : 1;
}
#endif
