// revise_task.h — which revisions mtr_test_revise (include/mtr_hip_test.h) takes: the ones the batch path hands to revise() and to mtr_k_revise_quads, and no
// others.  Plain C++17, nothing of HIP: the entry (test_entries.hip.inc) and a host-only program (tests/revise_task_check.cpp) compile the same function.
// A task is a read of the resident batch, the 13 scalar fields of a record in the order of RR / rr_t (rep_start, rep_end, repeat_len, period, copies, mat,
// mis, ins, del, k, G, MM, D) and a unit of `unit_len` bases.  What the batch path guarantees a revision (find_tandem_repeat_sub, handle_one_read.c:84-99,
// after a successful search_De_Bruijn_graph):
//   period    = the unit's length, 6 .. 499 (5 < period, period < MAX_PERIOD)
//   coverage  repeat_len / period in 5 .. 20
//   window    0 <= rep_start <= rep_end <= L: a traceback starts on a row of the search window and ends at or behind its start; rep_end = L is what a
//             repeat that runs to the end of its read gives under isolated semantics
//   counts    none negative, mat + mis + ins + del > 0 (the record's ratio divides by it), repeat_len > 0
//   k         2 .. 15, the k the search uses (k2_k_range)
//   size      every DP of the two rounds stays under WrapDPsize.  A revised unit has up to twice the bases, and the rounds' windows only shrink, so the
//             bound is taken at 2 period: (2 period + 1) rows + 2 period < WrapDPsize with rows = rep_end - rep_start + 1 (dp_size_ok's form; the CPU
//             oracle ends its process where a DP reaches the size, so nothing near it is let through)
#pragma once
#include <cstdint>
#include <string>

#define RVT_MIN_PERIOD 6
#define RVT_MAX_PERIOD 499
#define RVT_MIN_COVERAGE 5
#define RVT_MAX_COVERAGE 20
#define RVT_MIN_K 2
#define RVT_MAX_K 15
#define RVT_MAX_TASKS 4096            // what the entry's lists hold

// "" = eligible; else the reason (the caller names the task)
inline std::string rvt_refusal(int32_t rd, int32_t n_reads, const int32_t *lens, const int32_t *rr, int64_t unit_len, long long wrap_dp_size)
{
    if (rd < 0 || rd >= n_reads) return "read outside the batch";
    const long long L = lens[rd];
    const long long rs = rr[0], re = rr[1], repeat_len = rr[2], period = rr[3], k = rr[9];
    if (period < RVT_MIN_PERIOD || period > RVT_MAX_PERIOD) return "period outside 6..499";
    if (unit_len != period) return "the unit's length is not the period";
    if (rs < 0 || re < rs || re > L) return "window outside 0 <= rep_start <= rep_end <= L";
    if (rr[5] < 0 || rr[6] < 0 || rr[7] < 0 || rr[8] < 0 || (long long)rr[5] + rr[6] + rr[7] + rr[8] <= 0 || repeat_len <= 0) return "non-positive counts";
    const long long coverage = repeat_len / period;
    if (coverage < RVT_MIN_COVERAGE || coverage > RVT_MAX_COVERAGE) return "coverage outside 5..20";
    if (k < RVT_MIN_K || k > RVT_MAX_K) return "k outside 2..15";
    if ((2 * period + 1) * (re - rs + 1) + 2 * period >= wrap_dp_size) return "period x rows beyond WrapDPsize";
    return std::string();
}
