// dp_task_plan_check.cpp — the layouts and sizes the DP hosts hand to the device (mtr_amd/csrc/dp_task_plan.h), as a program of its own (the form
// a sanitizer build runs).  No GPU test sees these figures: a wrong one is a read or a write outside a buffer, which a kernel may survive.
//   the task table   its columns are written through and read back from the flat buffer against the order written out here, in a buffer of
//                    exactly the ints the hosts allocate (the address sanitizer watches the ends); the staging form and the device form -
//                    the same function over another base - must give the same offsets.
//   the lane slots   against a brute-force construction, bucket by bucket.
//   the five-launch plan   against the two formulas the hosts had before they shared it, restated here one statement after the other: the
//                    search's (L_lane, L_first, l_umax) and loci_round's (lane_len, u_wave or u_all, tasks / 64 + slots * MLO_N_CLASSES).
#include "../mtr_amd/csrc/dp_task_plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng >> 4; }      // xorshift32
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static long g_checks = 0;
static std::string g_case;
template <typename A, typename B> static void same(const std::string &what, A got, B want)
{
    g_checks++;
    if ((long long)got != (long long)want) {
        fprintf(stderr, "FAIL (%s): %s\n  header: %lld\n  model:  %lld\n", g_case.c_str(), what.c_str(), (long long)got, (long long)want);
        exit(1);
    }
}
static void hold(const std::string &what, bool ok) { same(what, ok ? 1 : 0, 1); }

// ---- the task table ----
// read | start | end | gain | mismatch | indel | unit_off (nt + 1), then group_off (ng + 1) when there are groups (ng > 0)
static void check_table(size_t nt, size_t ng)
{
    const size_t ints = ng > 0 ? dp_task_ints(nt, ng) : dp_task_ints(nt);
    same("ints of the table", ints, nt * 6 + (nt + 1) + (ng > 0 ? ng + 1 : 0));
    std::vector<int32_t> stage(ints, -1), device(ints, -1);
    const DpTaskTable<int32_t> s = dp_task_table<int32_t>(stage.data(), nt);
    const DpTaskTable<const int32_t> d = dp_task_table<const int32_t>(device.data(), nt);
    int32_t *const col[8] = { s.read, s.start, s.end, s.gain, s.mism, s.indel, s.unit_off, s.group_off };
    const int32_t *const dcol[8] = { d.read, d.start, d.end, d.gain, d.mism, d.indel, d.unit_off, d.group_off };
    const size_t len[8] = { nt, nt, nt, nt, nt, nt, nt + 1, ng > 0 ? ng + 1 : 0 };
    size_t at = 0;                                                        // the columns one behind the other, in the order above
    for (int c = 0; c < 8; c++) {
        same("column " + std::to_string(c) + " begins", col[c] - stage.data(), at);
        same("column " + std::to_string(c) + ": staging and device form", dcol[c] - device.data(), col[c] - stage.data());
        for (size_t i = 0; i < len[c]; i++) {
            hold("column " + std::to_string(c) + " is written once", col[c][i] == -1);          // disjoint: nobody was here before
            col[c][i] = (int32_t)(c * 1000003 + (int)i);
        }
        at += len[c];
    }
    same("the columns fill the table", at, ints);
    at = 0;
    for (int c = 0; c < 8; c++) for (size_t i = 0; i < len[c]; i++, at++) same("flat position " + std::to_string(at), stage[at], c * 1000003 + (int)i);
    if (ng == 0) same("group_off of a table without groups is its end", s.group_off - stage.data(), dp_task_ints(nt));
}

// ---- the scratch of a code matrix ----
static size_t model_align256(size_t x) { return (x + 255) / 256 * 256; }
static void check_matrix(size_t cells)
{
    const size_t b = dp_matrix_bytes(cells);
    same("matrix bytes", b, model_align256(cells + 256));
    hold("matrix bytes: the cells, the slack, whole 256-byte lines", b >= cells + 256 && b % 256 == 0 && b < cells + 512);
}

// ---- the lane slots ----
static int model_bucket(int U) { return U <= 4 ? 0 : U <= 8 ? 1 : U <= 16 ? 2 : 3; }
static void check_lane_slots(const std::vector<int32_t> &unit_off, int S, int lane_max, const LaneSlots &ls)
{
    std::vector<int32_t> q_slot; int q_first[5], l_umax[4] = { 0, 0, 0, 0 }, u_all = 0, u_wave = 0;
    std::vector<bool> has_lane((size_t)S, false);                          // the model's own assignment: u_wave is the longest motif WITHOUT a lane slot
    for (int k = 0; k < 4; k++) {
        q_first[k] = (int)q_slot.size();
        for (int slot = 0; slot < S; slot++) {
            const int U = unit_off[(size_t)slot + 1] - unit_off[(size_t)slot];
            if (U <= lane_max && model_bucket(U) == k) { q_slot.push_back(slot); has_lane[(size_t)slot] = true; if (U > l_umax[k]) l_umax[k] = U; }
        }
    }
    q_first[4] = (int)q_slot.size();
    same("lane slots", ls.q_slot.size(), q_slot.size());
    same("slots", ls.slot_q.size(), (size_t)S);
    for (size_t q = 0; q < q_slot.size(); q++) { same("q_slot", ls.q_slot[q], q_slot[q]); same("slot_q of a lane slot", ls.slot_q[(size_t)q_slot[q]], q); }
    for (int slot = 0; slot < S; slot++) {
        const int U = unit_off[(size_t)slot + 1] - unit_off[(size_t)slot];
        if (U > u_all) u_all = U;
        if (!has_lane[(size_t)slot]) { same("slot_q of a wave slot", ls.slot_q[(size_t)slot], -1); if (U > u_wave) u_wave = U; }
    }
    for (int k = 0; k < 5; k++) same("q_first", ls.q_first[k], q_first[k]);
    for (int k = 0; k < 4; k++) same("l_umax", ls.l_umax[k], l_umax[k]);
    same("u_all", ls.u_all, u_all); same("u_wave", ls.u_wave, u_wave);
}

// ---- the five-launch plan ----
struct Model { bool on[5]; size_t per_wave[5], cells_cap[5]; int per_cu[5]; int64_t items[5]; };
// the context's pick_waves stands behind `pick`: this one writes down what it is asked, in order, and answers with figures of its own
struct Pick {
    struct Call { int64_t items; int per_cu; size_t per_wave; };
    std::vector<Call> *calls;
    int operator()(int64_t items, int per_cu, size_t per_wave, size_t *total) const
    {
        calls->push_back({ items, per_cu, per_wave });
        const int waves = 1 + (int)(items % 7);
        *total = (size_t)waves * per_wave + calls->size();
        return waves;
    }
};
static void check_plan(const DpLaunchPlan &p, const std::vector<Pick::Call> &calls, const Model &m)
{
    size_t c = 0, scratch = 0;
    for (int k = 0; k < 5; k++) {
        const std::string l = "launch " + std::to_string(k) + ": ";
        same(l + "present", p.waves[k] > 0, m.on[k]);
        if (!m.on[k]) { same(l + "no scratch when absent", p.per_wave[k], 0); continue; }
        hold(l + "picked in launch order", c < calls.size());
        same(l + "items", calls[c].items, m.items[k]); same(l + "per CU", calls[c].per_cu, m.per_cu[k]); same(l + "per_wave asked", calls[c].per_wave, m.per_wave[k]);
        same(l + "per_wave", p.per_wave[k], m.per_wave[k]); same(l + "cells_cap", p.cells_cap[k], m.cells_cap[k]);
        same(l + "waves", p.waves[k], 1 + (int)(m.items[k] % 7));
        c++;
        scratch = std::max(scratch, (size_t)p.waves[k] * m.per_wave[k] + c);
    }
    same("one pick per launch", calls.size(), c);
    same("the scratch is the largest total", p.scratch, scratch);
}
// mtr_search_motifs_device before the plan was shared, list building included: reads of lens[], motif slots of ulen[]
static void check_search(const std::vector<int> &lens_in, const std::vector<int> &ulen, int lane_max, int lane_rows)
{
    std::vector<int> lens = lens_in;
    std::sort(lens.begin(), lens.end(), [](int a, int b) { return a > b; });
    const int n = (int)lens.size();
    int n_long = 0;
    while (n_long < n && lens[(size_t)n_long] > lane_rows) n_long++;
    const long long L_first = lens[0], L_lane = n_long < n ? lens[(size_t)n_long] : 0;
    const int64_t groups = ((int64_t)(n - n_long) + 63) / 64;
    static const int bucket_ub[4] = { 4, 8, 16, 32 };
    int64_t l_entries[5] = { 0, 0, 0, 0, 0 }, l_items[5] = { 0, 0, 0, 0, 0 }; int l_umax[5] = { 0, 0, 0, 0, 0 };
    for (int U : ulen) {
        if (U <= lane_max && groups > 0) {
            int k = 0; while (bucket_ub[k] < U) k++;
            same("columns of a bucket", dp_bucket_ub(k), bucket_ub[k]); same("mdp_bucket", mdp_bucket(U), bucket_ub[k]);
            l_entries[k]++; l_items[k] += groups; l_umax[k] = std::max(l_umax[k], U);
        }
        const int64_t by_wave = U <= lane_max ? n_long : n;
        if (by_wave > 0) { l_entries[4]++; l_items[4] += by_wave; l_umax[4] = std::max(l_umax[4], U); }
    }
    Model m{};
    const size_t wave_cells = (size_t)L_first * (size_t)(l_umax[4] + 1);
    for (int k = 0; k < 5; k++) {
        if (l_entries[k] == 0) continue;
        m.on[k] = true; m.items[k] = l_items[k];
        m.per_wave[k] = k < 4 ? model_align256((size_t)L_lane * (size_t)((l_umax[k] + 3) >> 2) * 256) : model_align256(wave_cells + 256);
        m.per_cu[k] = k < 4 ? 16 : 8; m.cells_cap[k] = k < 4 ? 0 : wave_cells;
    }
    std::vector<Pick::Call> calls;
    const DpLaunchPlan p = dp_search_plan(L_lane, L_first, l_umax, l_items, Pick{ &calls });
    check_plan(p, calls, m);
}
// loci_round before the plan was shared: `tasks` windows of at most max_len bases over the motif slots of ulen[]
static void check_loci(const std::vector<int> &ulen, int lane_max, int lane_rows, int64_t tasks, int max_len)
{
    std::vector<int32_t> unit_off(1, 0);
    for (int U : ulen) unit_off.push_back(unit_off.back() + U);
    const int S = (int)ulen.size();
    const LaneSlots ls = lane_slots(unit_off, S, lane_max);
    check_lane_slots(unit_off, S, lane_max, ls);
    const int lane_len = std::min(max_len, lane_rows);
    const bool by_wave = ls.u_wave > 0 || max_len > lane_rows;
    const size_t wave_cells = (size_t)max_len * (size_t)((max_len > lane_rows ? ls.u_all : ls.u_wave) + 1);
    Model m{};
    for (int k = 0; k < 5; k++) {
        if (k < 4 ? ls.q_first[k] == ls.q_first[k + 1] : !by_wave) continue;
        m.on[k] = true;
        m.per_wave[k] = k < 4 ? model_align256((size_t)lane_len * (size_t)((ls.l_umax[k] + 3) >> 2) * 256) : model_align256(wave_cells + 256);
        m.items[k] = k < 4 ? tasks / 64 + (int64_t)(ls.q_first[k + 1] - ls.q_first[k]) * MLO_N_CLASSES : tasks;
        m.per_cu[k] = k < 4 ? 16 : 8; m.cells_cap[k] = k < 4 ? 0 : wave_cells;
    }
    std::vector<Pick::Call> calls;
    const DpLaunchPlan p = dp_loci_plan(ls, tasks, max_len, lane_rows, Pick{ &calls });
    check_plan(p, calls, m);
}
static void check_both(const std::vector<int> &lens, const std::vector<int> &ulen, int lane_max, int lane_rows)
{
    check_search(lens, ulen, lane_max, lane_rows);
    const int L = *std::max_element(lens.begin(), lens.end());
    check_loci(ulen, lane_max, lane_rows, (int64_t)lens.size() * (int64_t)ulen.size(), L);                       // round 0: every pair's whole read
    check_loci(ulen, lane_max, lane_rows, std::max<int64_t>(1, (int64_t)lens.size() / 3), std::max(1, L / 5));   // a later round: fewer, shorter windows
}

static int g_named = 0;
static void named(const std::string &name) { g_case = name; g_named++; }

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? atoi(argv[1]) : 300;
    const std::vector<int> reads70 = [] { std::vector<int> v; for (int i = 0; i < 70; i++) v.push_back(60 + 2 * i); return v; }();
    named("nt = 1"); check_table(1, 0);
    named("ng = 1"); check_table(5, 1);
    named("nt = 1, ng = 1"); check_table(1, 1);
    named("an empty bucket"); check_both(reads70, { 3, 12, 20, 40 }, 32, 16384);                       // nothing of 5..8 bases
    named("no wave path"); check_both(reads70, { 3, 7, 12, 20 }, 32, 16384);
    named("no lane path: no motif short enough"); check_both(reads70, { 3, 7, 12, 20, 40 }, 0, 16384);
    named("no lane path: every motif long"); check_both(reads70, { 33, 40, 499 }, 32, 16384);
    for (int U : { 4, 5, 8, 9, 16, 17, 32 }) { named("umax = " + std::to_string(U)); check_both(reads70, { 1, U }, 32, 16384); check_both(reads70, { U }, U, 100); }
    named("lane rows of 0"); check_both(reads70, { 3, 7, 12, 20, 40 }, 32, 0);
    named("lane rows of 0 under a lane launch");                                                       // the plan itself, whatever the host would ask
    {
        const int umax[5] = { 4, 8, 16, 32, 40 }; const int64_t items[5] = { 1, 1, 1, 1, 1 };
        std::vector<Pick::Call> calls;
        const DpLaunchPlan p = dp_search_plan(0, 100, umax, items, Pick{ &calls });
        for (int k = 0; k < 4; k++) same("per_wave of no rows", p.per_wave[k], 0);
        same("the wave launch", p.per_wave[4], model_align256(100 * 41 + 256));
    }
    named("lane rows split the reads"); check_both(reads70, { 3, 7, 12, 20, 40 }, 32, 100);
    named("one read, one motif"); check_both({ 1 }, { 1 }, 32, 16384);
    for (size_t cells : { (size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)200000000 }) { named("matrix of " + std::to_string(cells) + " cells"); check_matrix(cells); }
    const int n_named = g_named;
    for (int r = 0; r < n_random; r++) {
        g_case = "random shape " + std::to_string(r);
        check_table((size_t)rnd_in(1, 300), r % 3 == 0 ? 0 : (size_t)rnd_in(1, 40));
        check_matrix((size_t)rnd_in(0, 1 << 20));
        std::vector<int> lens((size_t)rnd_in(1, 200)), ulen((size_t)rnd_in(1, 12));
        const int span = r % 4 == 0 ? 20000 : 400;
        for (int &L : lens) L = rnd_in(1, span);
        for (int &U : ulen) U = r % 5 == 0 ? rnd_in(1, 499) : rnd_in(1, 36);
        check_both(lens, ulen, r % 7 == 0 ? rnd_in(0, 32) : 32, r % 2 == 0 ? 16384 : rnd_in(0, span));
    }
    printf("ok: %d named cases, %d random shapes, %ld checks\n", n_named, n_random, g_checks);
    return 0;
}
