// dp_task_plan_check.cpp — the layouts and sizes the DP hosts hand to the device (mtr_amd/csrc/dp_task_plan.h), as a program of its own (the form
// a sanitizer build runs).  No GPU test sees these figures: a wrong one is a read or a write outside a buffer, which a kernel may survive.
//   the task table   its columns are written through and read back from the flat buffer against the order written out here, in a buffer of
//                    exactly the ints the hosts allocate (the address sanitizer watches the ends); the staging form and the device form -
//                    the same function over another base - must give the same offsets.
//   the lane slots   against a brute-force construction, bucket by bucket.
//   the five-launch plan   against the two formulas the hosts had before they shared it, restated here one statement after the other: the
//                    search's (L_lane, L_first, l_umax) and loci_round's (lane_len, u_wave or u_all, tasks / 64 + slots * MLO_N_CLASSES).
//   a round of the locus search   every buffer's bytes and every slice's place against the locus search's and the genotype's former statements, the
//                    slices written through in heap buffers of exactly those bytes; the refusal where the bins outgrow an int32.
#include "../mtr_amd/csrc/dp_task_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// ---- one round of the locus search ----
// a buffer of exactly `bytes` on the heap (the address sanitizer watches its ends), every byte 0xff; a slice is written through element by element,
// each found untouched (disjoint: nobody was here before) and read back at the end
struct Heap {
    uint8_t *p; size_t bytes, written = 0;
    explicit Heap(size_t n) : p((uint8_t *)malloc(n)), bytes(n) { if (!p) { fprintf(stderr, "out of memory\n"); exit(1); } memset(p, 0xff, n); }
    ~Heap() { free(p); }
    Heap(const Heap &) = delete;
    template <typename T> void slice(const std::string &what, size_t at, size_t n, int tag)
    {
        T *s = (T *)p + at;
        hold(what + " is aligned to its elements", (uintptr_t)s % sizeof(T) == 0);
        for (size_t i = 0; i < n; i++) { hold(what + " is written once", s[i] == (T)-1); s[i] = (T)(tag * 1000003 + (int)i); }
        for (size_t i = 0; i < n; i++) same(what + " reads back", s[i], (T)(tag * 1000003 + (int)i));
        written += n * sizeof(T);
    }
};
// the two hosts before they shared the layout, one statement after the other: mtr_search_motif_loci_device over its d_ml_* buffers, then
// genotype_align_tables over its d_gt_* (MS_RES = 9 ints a task, LOCI_STATE = 5 words, five counters)
static void check_round(size_t sS, size_t nq, size_t nt)
{
    LociRoundLayout l; std::string err;
    hold("the layout is given", loci_round_layout(sS, nq, nt, l, err) && err.empty());
    const size_t nb = nq * 177;
    same("bins", l.nb, nb); same("MLO_N_CLASSES", MLO_N_CLASSES, 177); same("ints a result", LOCI_RES_INTS, 9); same("state words", LOCI_STATE_INTS, 5);
    // the locus search
    const size_t ml_i32 = (2 * sS + 1 + nq + 1) * 4;
    const size_t ml_i64 = sS * 8;
    const size_t ml_bin32 = (2 * nb + 1) * 4;
    const size_t ml_bin64 = 2 * (nb + 1) * 8;
    const size_t ml_state = 5 * 4;
    const size_t ml_counter = 5 * 8;
    const size_t ml_slot_q = sS + 1;                                      // d_slot_q = d_uoff + sS + 1
    const size_t ml_q_slot = ml_slot_q + sS;                              // d_q_slot = d_slot_q + sS
    const size_t ml_groups = nb;                                          // a.groups = a.hist + nb
    const size_t ml_gfirst = nb + 1;                                      // a.gfirst = a.tfirst + nb + 1
    const size_t ml_task32 = 4 * nt * 4;
    const size_t ml_res = nt * 9 * 4;
    const size_t ml_trank = nt;                                           // a.trank = a.tbin + nt
    const size_t ml_sorted = ml_trank + nt;                               // a.sorted = a.trank + nt
    const size_t ml_wlist = ml_sorted + nt;                               // a.wlist = a.sorted + nt
    // the genotype
    const size_t gt_i32 = (3 * sS + 2) * 4;                               // the bound: q_slot's address is kept from before nq is known
    const size_t gt_i64 = sS * 8;
    const size_t gt_slot_q = sS + 1;
    const size_t gt_q_slot = gt_slot_q + sS;
    const size_t gt_bin32 = (2 * nb + 1) * 4;
    const size_t gt_bin64 = 2 * (nb + 1) * 8;
    const size_t gt_counter = 5 * 8;
    const size_t gt_task32 = 4 * nt * 4;
    const size_t gt_res = nt * 9 * 4;
    const size_t gt_state = 5 * 4;
    const size_t gt_groups = nb, gt_gfirst = nb + 1, gt_trank = nt, gt_sorted = gt_trank + nt, gt_wlist = gt_sorted + nt;
    same("i32: the genotype's bound", l.i32_bytes, gt_i32);
    hold("i32: the locus search's, grown by at most S - nq ints", l.i32_bytes >= ml_i32 && l.i32_bytes - ml_i32 <= (sS - nq) * 4);
    same("i64 (locus search)", l.i64_bytes, ml_i64); same("i64 (genotype)", l.i64_bytes, gt_i64);
    same("bin32 (locus search)", l.bin32_bytes, ml_bin32); same("bin32 (genotype)", l.bin32_bytes, gt_bin32);
    same("bin64 (locus search)", l.bin64_bytes, ml_bin64); same("bin64 (genotype)", l.bin64_bytes, gt_bin64);
    same("task32 (locus search)", l.task32_bytes, ml_task32); same("task32 (genotype)", l.task32_bytes, gt_task32);
    same("res (locus search)", l.res_bytes, ml_res); same("res (genotype)", l.res_bytes, gt_res);
    same("state (locus search)", l.state_bytes, ml_state); same("state (genotype)", l.state_bytes, gt_state);
    same("counter (locus search)", l.counter_bytes, ml_counter); same("counter (genotype)", l.counter_bytes, gt_counter);
    same("slot_q (locus search)", l.slot_q, ml_slot_q); same("slot_q (genotype)", l.slot_q, gt_slot_q);
    same("q_slot (locus search)", l.q_slot, ml_q_slot); same("q_slot (genotype)", l.q_slot, gt_q_slot);
    same("groups (locus search)", l.groups, ml_groups); same("groups (genotype)", l.groups, gt_groups);
    same("gfirst (locus search)", l.gfirst, ml_gfirst); same("gfirst (genotype)", l.gfirst, gt_gfirst);
    same("trank (locus search)", l.trank, ml_trank); same("trank (genotype)", l.trank, gt_trank);
    same("sorted (locus search)", l.sorted, ml_sorted); same("sorted (genotype)", l.sorted, gt_sorted);
    same("wlist (locus search)", l.wlist, ml_wlist); same("wlist (genotype)", l.wlist, gt_wlist);
    const LociRoundLayout s0 = loci_slot_layout(sS);                      // what the genotype takes before it knows nq
    same("the slots alone: i32", s0.i32_bytes, l.i32_bytes); same("the slots alone: i64", s0.i64_bytes, l.i64_bytes);
    same("the slots alone: slot_q", s0.slot_q, l.slot_q); same("the slots alone: q_slot", s0.q_slot, l.q_slot);
    // every slice written through, in buffers of exactly the layout's bytes
    Heap i32(l.i32_bytes), i64(l.i64_bytes), bin32(l.bin32_bytes), bin64(l.bin64_bytes), task32(l.task32_bytes), res(l.res_bytes), state(l.state_bytes), counter(l.counter_bytes);
    i32.slice<int32_t>("unit_off", 0, sS + 1, 1); i32.slice<int32_t>("slot_q", l.slot_q, sS, 2); i32.slice<int32_t>("q_slot", l.q_slot, nq, 3);
    i64.slice<uint64_t>("bits", 0, sS, 4);
    bin32.slice<int32_t>("hist", 0, nb, 5); bin32.slice<int32_t>("groups", l.groups, nb, 6);
    bin64.slice<int64_t>("tfirst", 0, nb + 1, 7); bin64.slice<int64_t>("gfirst", l.gfirst, nb + 1, 8);
    task32.slice<int32_t>("tbin", 0, nt, 9); task32.slice<int32_t>("trank", l.trank, nt, 10); task32.slice<int32_t>("sorted", l.sorted, nt, 11); task32.slice<int32_t>("wlist", l.wlist, nt, 12);
    res.slice<int32_t>("res", 0, nt * 9, 13); state.slice<int32_t>("state", 0, 5, 14); counter.slice<unsigned long long>("counter", 0, 5, 15);
    same("i32: room for q_slot up to S is all that is left", i32.bytes - i32.written, (sS - nq + 1) * 4);
    same("bin32: one int over", bin32.bytes - bin32.written, 4);
    for (const Heap *h : { &i64, &bin64, &task32, &res, &state, &counter }) same("the slices fill the buffer", h->written, h->bytes);
}
static void check_round_refusal()
{
    LociRoundLayout l; std::string err;
    const size_t fits = (size_t)INT32_MAX / 177, over = fits + 1;          // 12 132 675 lane slots are the most whose bins an int32 counts
    hold("the most lane slots that fit", loci_round_layout(fits, fits, 1, l, err) && err.empty() && l.nb == fits * 177);
    hold("one more is refused", !loci_round_layout(over, over, 1, l, err));
    hold("in the hosts' words", err == std::to_string(over) + " short motifs are more than the bins take");
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
    for (size_t S : { (size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)65 })
        for (size_t nq : S == 1 ? std::vector<size_t>{ 0, 1 } : std::vector<size_t>{ 0, 1, S })             // nq = 0, 1 and S
            for (size_t nt : { (size_t)1, (size_t)63, (size_t)64, (size_t)65 }) {
                named("a round of S = " + std::to_string(S) + ", nq = " + std::to_string(nq) + ", nt = " + std::to_string(nt)); check_round(S, nq, nt);
            }
    named("more short motifs than the bins take"); check_round_refusal();
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
