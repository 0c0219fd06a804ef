// dp_task_plan.h — the layouts and sizes the hosts of the wrap-around DP kernels hand to the device, each stated once.  Plain C++, nothing of
// HIP: a wrong figure here is an out-of-bounds access on the GPU, not a failing assertion, so tests/dp_task_plan_check.cpp holds them to the formulas one by one.
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "mtr_common.h"
#include "motif_dp.h"
#include "motif_loci.h"
// the task table: read | start | end | gain | mismatch | indel | unit_off (nt + 1) [| group_off (ng + 1)] in one int32 buffer, a host staging vector's or the device's
template <typename Int> struct DpTaskTable { Int *read, *start, *end, *gain, *mism, *indel, *unit_off, *group_off; };
static inline size_t dp_task_ints(size_t nt) { return 7 * nt + 1; }
static inline size_t dp_task_ints(size_t nt, size_t ng) { return dp_task_ints(nt) + ng + 1; }       // with the groups of mtr_test_wrap_dp_pass
template <typename Int> static inline DpTaskTable<Int> dp_task_table(Int *base, size_t nt) { return { base, base + nt, base + 2 * nt, base + 3 * nt, base + 4 * nt, base + 5 * nt, base + 6 * nt, base + dp_task_ints(nt) }; }
// the scratch of a wavefront that holds one code matrix of `cells` bytes; + slack: the traceback's dword loads read a few bytes past a row
static inline size_t dp_matrix_bytes(size_t cells) { return mtrc_align(cells + 256, 256); }

// the lane slots of S motif slots, numbered bucket by bucket: bucket k's bins are q_first[k] * MLO_N_CLASSES .. q_first[k + 1] * MLO_N_CLASSES
#define DP_LANE_BUCKETS 4                               // bucket k takes the motifs that run with dp_bucket_ub(k) columns
#define DP_LAUNCHES 5                                   // the four lane buckets' launches, then the wave path's
static inline int dp_bucket_ub(int k) { return 4 << k; }                                            // 4, 8, 16, 32: mdp_bucket's values
struct LaneSlots {
    std::vector<int32_t> slot_q, q_slot;
    int q_first[5] = { 0, 0, 0, 0, 0 }, l_umax[4] = { 0, 0, 0, 0 }, u_all = 0, u_wave = 0;      // u_wave: the longest motif no lane takes
};
static inline LaneSlots lane_slots(const std::vector<int32_t> &unit_off, int S, int lane_max)
{
    LaneSlots ls; ls.slot_q.assign((size_t)S, -1);
    for (int k = 0; k <= DP_LANE_BUCKETS; k++) {                     // k = 4: no bucket, the longest motifs (lane_max <= MDP_MAX_U: every shorter one has a bucket)
        ls.q_first[k] = (int)ls.q_slot.size();
        for (int slot = 0; slot < S; slot++) {
            const int U = unit_off[(size_t)slot + 1] - unit_off[(size_t)slot];
            if (k == DP_LANE_BUCKETS) { ls.u_all = std::max(ls.u_all, U); if (U > lane_max) ls.u_wave = std::max(ls.u_wave, U); }
            else if (U <= lane_max && mdp_bucket(U) == dp_bucket_ub(k)) { ls.slot_q[(size_t)slot] = (int32_t)ls.q_slot.size(); ls.q_slot.push_back(slot); ls.l_umax[k] = std::max(ls.l_umax[k], U); }
        }
    }
    return ls;
}
// The five launches of the known-motif kernels.  k < 4: bucket k's lane kernel, a wavefront holds rows x dwords x 64 lanes of cells, 16 per CU, no cell cap; k = 4: the
// wave kernel, one code matrix a wavefront, 8 per CU, capped at its cells.  The scratch is shared: the largest total.  A launch without items does not run (waves 0) - the
// hosts used to launch the wave kernel over 0 tasks, which no caller reaches (every one has tasks > 0).  pick(items, per_cu, per_wave, &total): the context's pick_waves.
struct DpLaunchPlan { size_t per_wave[DP_LAUNCHES], cells_cap[DP_LAUNCHES], scratch; int waves[DP_LAUNCHES]; };
template <typename Pick> static inline DpLaunchPlan dp_launch_plan(size_t lane_rows, const int lane_umax[DP_LANE_BUCKETS], size_t wave_cells, const int64_t items[DP_LAUNCHES], Pick pick)
{
    DpLaunchPlan p{};
    for (int k = 0; k < DP_LAUNCHES; k++) {
        if (items[k] <= 0) continue;
        const bool lanes = k < DP_LANE_BUCKETS;
        p.per_wave[k] = lanes ? mtrc_align(lane_rows * (size_t)mdp_dwords(lane_umax[k]) * 256, 256) : dp_matrix_bytes(wave_cells);
        p.cells_cap[k] = lanes ? 0 : wave_cells;
        size_t total = 0; p.waves[k] = pick(items[k], lanes ? 16 : 8, p.per_wave[k], &total); p.scratch = std::max(p.scratch, total);
    }
    return p;
}
template <typename Pick> static inline DpLaunchPlan dp_search_plan(long long L_lane, long long L_first, const int l_umax[DP_LAUNCHES], const int64_t l_items[DP_LAUNCHES], Pick pick)
{ return dp_launch_plan((size_t)L_lane, l_umax, (size_t)L_first * (size_t)(l_umax[4] + 1), l_items, pick); }      // the search's: lanes take reads of up to L_lane bases, waves up to L_first
template <typename Pick> static inline DpLaunchPlan dp_loci_plan(const LaneSlots &ls, int64_t tasks, int max_len, int lane_rows, Pick pick)
{   // a round's of the locus search: `tasks` windows of at most max_len bases, the lanes take those of up to lane_rows (their items are a bound)
    int64_t items[DP_LAUNCHES];
    for (int k = 0; k < DP_LANE_BUCKETS; k++) items[k] = ls.q_first[k] == ls.q_first[k + 1] ? 0 : tasks / 64 + (int64_t)(ls.q_first[k + 1] - ls.q_first[k]) * MLO_N_CLASSES;
    items[4] = ls.u_wave > 0 || max_len > lane_rows ? tasks : 0;
    return dp_launch_plan((size_t)std::min(max_len, lane_rows), ls.l_umax, (size_t)max_len * (size_t)((max_len > lane_rows ? ls.u_all : ls.u_wave) + 1), items, pick);
}

// One round of the locus search's kernels (loci_round) over S motif slots, nq of them lane slots, and nt tasks: every buffer's bytes and, counted in
// the buffer's own elements, where each slice begins.  The locus search and the genotype both size and slice by this (LociRoundBufs).
//   i32     unit_off (S + 1) | slot_q (S) | q_slot (nq, with room for S: the genotype keeps q_slot's address from before nq is known)         i64   bits (S)
//   bin32   hist (nb) | groups (nb), one int over; nb = nq * MLO_N_CLASSES bins         bin64   tfirst (nb + 1) | gfirst (nb + 1)
//   task32  tbin | trank | sorted | wlist, nt each       res   LOCI_RES_INTS a task       state   LOCI_STATE_INTS words       counter   8 bytes a launch
#define LOCI_RES_INTS 9                                 // MS_RES (motif_search.hip.inc)
#define LOCI_STATE_INTS 5                               // LOCI_STATE (motif_loci.hip.inc)
struct LociRoundLayout { size_t nb, i32_bytes, i64_bytes, bin32_bytes, bin64_bytes, task32_bytes, res_bytes, state_bytes, counter_bytes, slot_q, q_slot, groups, gfirst, trank, sorted, wlist; };
static inline bool loci_round_layout(size_t S, size_t nq, size_t nt, LociRoundLayout &l, std::string &err)
{
    if ((int64_t)nq * MLO_N_CLASSES > (int64_t)INT32_MAX) { err = std::to_string(nq) + " short motifs are more than the bins take"; return false; }
    const size_t nb = nq * MLO_N_CLASSES;
    l = { nb, (3 * S + 2) * 4, S * 8, (2 * nb + 1) * 4, 2 * (nb + 1) * 8, 4 * nt * 4, nt * LOCI_RES_INTS * 4, LOCI_STATE_INTS * 4, DP_LAUNCHES * 8,
          S + 1, 2 * S + 1, nb, nb + 1, nt, 2 * nt, 3 * nt };
    return true;
}
// what S alone decides, for a host that does not know nq yet: the slot ints' bound, slot_q's and q_slot's places, the bits
static inline LociRoundLayout loci_slot_layout(size_t S) { LociRoundLayout l; std::string none; loci_round_layout(S, 0, 0, l, none); return l; }
