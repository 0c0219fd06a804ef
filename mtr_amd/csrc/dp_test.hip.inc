// dp_test.hip.inc — test kernels that run ONE chosen forward pass of the wrap-around DP, with its tracebacks, on groups of tasks the caller
// chose (mtr_test_wrap_dp_pass, include/mtr_hip_test.h).  A group is the set of DPs that share one forward pass.  In the batch path the unit
// search decides which windows, units, row counts and group compositions a pass sees; here a test does.
//
// Nothing of a pass is written here: the kernels call the device functions the batch path calls (dp_wrap2 / dp_wrap, dp_forward2p_q4,
// dp_forward2p_g16<C>, st_fwd2p_oct, st_fwd1p_four, st_fwd1p_any, dp_traceback<0, .>) with the geometry the batch path gives them (cell blocks by DPQ_DP_BYTES /
// DPQP_DP_BYTES, wlim from the batch's packed words), under the launch bounds of the kernel they stand for.  What the batch path does AFTER a
// traceback (apply_dp, the choice between the two parameter sets) is left out on purpose: a test sees each parameter set's eight integers.
// The host refuses every task the batch path would not hand to the pass (mtr_abi.hip), so nothing below re-checks eligibility.
#pragma once
#include "dp_wrap.hip.inc"

struct DpPassArgs {
    DpTestArgs t;                  // the task arrays of mtr_k_dp_test; t.out8 holds 16 integers per task: [task][parameter set][8]
    int32_t pass, n_groups;
    const int32_t *group_off;      // group g = tasks group_off[g] .. group_off[g + 1]
    long long packed_words;        // as K2Args: words readable at b.packed
};

DEVINL void dpt_clear(DpRes &o) { o.stop_i = 0; o.end_i = 0; o.mat = o.mis = o.ins = o.del = o.scanned = 0; o.end_j = 0; }
// the eight integers of mtr_k_dp_test, window convention included
DEVINL void dpt_store(const DpPassArgs &a, int task, int p, int qs, int U, const DpRes &o)
{
    if (lane_id() == 0) {
        int32_t *r = a.t.out8 + ((size_t)task * 2 + (size_t)p) * 8;
        r[0] = qs + o.stop_i + 1; r[1] = qs + o.end_i; r[2] = o.end_i - o.stop_i; r[3] = U > 0 ? o.scanned / U : 0;
        r[4] = o.mat; r[5] = o.mis; r[6] = o.ins; r[7] = o.del;
    }
}
// the traceback of one DP of a pass from the pass's best cell, as every caller of dp_traceback<0, .> guards it
template <int FMT>
DEVINL void dpt_traceback(const DpPassArgs &a, const uint32_t *pk, int qs, int U, const uint8_t *cells, int psel, int rstride, const int (&best)[3],
                          DpRes &o, unsigned long long *wc)
{
    dpt_clear(o);
    const int bv = uni(best[0]), bi = uni(best[1]), bj = uni(best[2]);
    if (bv > 0) {
        dp_traceback<0, FMT>(pk, qs, U, cells, psel, rstride, bi, bj, nullptr, nullptr, nullptr, o, wc);
        if (o.stop_i < 0) { dpt_clear(o); set_status(a.t.status, DEV_ERR_DP_TOO_LARGE); }
    }
}

// MTR_TEST_PASS_WAVE2P, MTR_TEST_PASS_Q4: what st_dp2_waves_body runs, one alignment (or up to four units <= 16 over one window) per wavefront
__global__ __launch_bounds__(64, MTR_DP2_WAVES_PER_SIMD) void mtr_k_dp_test_waves(DpPassArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    uint8_t *sc = a.t.scratch + (size_t)blockIdx.x * a.t.scratch_per_wave;
    for (;;) {
        const int grp = next_work_item(a.t.work_counter);
        if (grp >= a.n_groups) break;
        const int t0 = uni(a.group_off[grp]), n = uni(a.group_off[grp + 1]) - t0;
        const int rd = uni(a.t.read_idx[t0]);
        const uint32_t *pk = a.t.b.packed + uni64(a.t.b.woff[rd]);
        const int qs = uni(a.t.qs[t0]), rows = uni(a.t.qe[t0]) - qs + 1;
        if (a.pass == MTR_TEST_PASS_WAVE2P) {
            // dp_two_params_unit's decision: both parameter sets in one forward pass where dp_wrap2 takes them, else one after the other
            const int uo = uni(a.t.unit_off[t0]), U = uni(a.t.unit_off[t0 + 1]) - uo;
            const uint8_t *unit = a.t.units + uo;
            DpRes o[2];
            bool ok;
            if (dp_wrap2_fits(rows, U, a.t.dp16_max_rows)) ok = dp_wrap2(pk, qs, rows, unit, U, 1, 1, 3, 1, 3, 1, sc, a.t.cells_cap, o, s_cnt, a.t.dp16_max_rows);
            else {
                ok = dp_wrap(pk, qs, rows, unit, U, 1, 1, 3, sc, a.t.cells_cap, 0, nullptr, nullptr, nullptr, o[0], s_cnt, a.t.dp16_max_rows);
                ok = dp_wrap(pk, qs, rows, unit, U, 1, 3, 1, sc, a.t.cells_cap, 0, nullptr, nullptr, nullptr, o[1], s_cnt, a.t.dp16_max_rows) && ok;
            }
            if (!ok) set_status(a.t.status, DEV_ERR_DP_TOO_LARGE);
            dpt_store(a, t0, 0, qs, U, o[0]); dpt_store(a, t0, 1, qs, U, o[1]);
        } else {
            // dp_two_params_q4's geometry: the matrices one behind the other, row stride = the unit's length; a DP that is not there has one column and no cells
            Dp4 q; q.n = n;
            size_t off = 0;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const bool on = g < n;
                const int tg = t0 + (on ? g : 0);
                const int uo = uni(a.t.unit_off[tg]);
                q.U[g] = on ? uni(a.t.unit_off[tg + 1]) - uo : 1; q.unit[g] = a.t.units + uo;
                q.off[g] = on ? off : 0;
                if (on) off += (size_t)rows * (size_t)q.U[g];
            }
            int best[4][2][3];
            dp_forward2p_q4(pk, qs, rows, q, 1, 1, 3, 1, 3, 1, sc, best);
            wave_sync_mem();
#pragma unroll
            for (int g = 0; g < 4; g++) {
                if (g < n) {
                    for (int p = 0; p < 2; p++) {
                        DpRes o;
                        dpt_traceback<1>(a, pk, qs, q.U[g], sc + q.off[g], p, q.U[g], best[g][p], o, s_cnt);
                        dpt_store(a, t0 + g, p, qs, q.U[g], o);
                        loop_join();
                    }
                }
            }
        }
        wave_sync_mem();                                   // the next group's forward pass overwrites the cells the tracebacks have read
        loop_join();
    }
    wc_flush(s_cnt, a.t.counters);
}

// MTR_TEST_PASS_QUAD2P: st_quad_run<C>'s forward pass and tracebacks for groups of one DPQ_COLS class (the host launches the class's kernel)
template <int C>
__global__ __launch_bounds__(64, 4) void mtr_k_dp_test_quads(DpPassArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    uint8_t *cells = a.t.scratch + (size_t)blockIdx.x * a.t.scratch_per_wave;
    for (;;) {
        const int grp = next_work_item(a.t.work_counter);
        if (grp >= a.n_groups) break;
        const int t0 = uni(a.group_off[grp]), n = uni(a.group_off[grp + 1]) - t0;
        DpQuad q; q.n = n;
        int maxrows = 0;
#pragma unroll
        for (int g = 0; g < 4; g++) {                       // (a slot that is empty repeats the first member with no rows, as mtr_k_dp2_quads fills it)
            const int tg = t0 + (g < n ? g : 0);
            const int rd = uni(a.t.read_idx[tg]), uo = uni(a.t.unit_off[tg]);
            q.pk[g] = a.t.b.packed + uni64(a.t.b.woff[rd]);
            q.wlim[g] = a.packed_words - uni64(a.t.b.woff[rd]);
            q.base[g] = uni(a.t.qs[tg]); q.rows[g] = g < n ? uni(a.t.qe[tg]) - q.base[g] + 1 : 0;
            q.U[g] = uni(a.t.unit_off[tg + 1]) - uo; q.unit[g] = a.t.units + uo;
            q.G[g] = 1; q.MM[g] = 1; q.D[g] = 1;
            maxrows = q.rows[g] > maxrows ? q.rows[g] : maxrows;
        }
        int best[4][2][3];
        dp_forward2p_g16<C>(q, 1, 1, 3, 1, 3, 1, cells, maxrows, best);
        wave_sync_mem();
#pragma unroll
        for (int g = 0; g < 4; g++) {
            if (g < n) {
                for (int p = 0; p < 2; p++) {
                    DpRes o;
                    dpt_traceback<1>(a, q.pk[g], q.base[g], q.U[g], cells + g * DPQ_DP_BYTES(C, maxrows), p, DPQ_ROW_BYTES(C), best[g][p], o, s_cnt);
                    dpt_store(a, t0 + g, p, q.base[g], q.U[g], o);
                    loop_join();
                }
            }
        }
        wave_sync_mem();
        loop_join();
    }
    wc_flush(s_cnt, a.t.counters);
}

// MTR_TEST_PASS_OCT2P: st_oct_run's forward pass and tracebacks for groups of up to eight units of at most ST_OUMAX bases (every lane fills in ITS DP; an
// empty slot repeats the first member with no rows, as st_oct_run fills it)
__global__ __launch_bounds__(64, 4) void mtr_k_dp_test_octs(DpPassArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    const int lane = lane_id();
    if (lane < CNT_N) s_cnt[lane] = 0ull;
    uint8_t *cells = a.t.scratch + (size_t)blockIdx.x * a.t.scratch_per_wave;
    for (;;) {
        const int grp = next_work_item(a.t.work_counter);
        if (grp >= a.n_groups) break;
        const int t0 = uni(a.group_off[grp]), n = uni(a.group_off[grp + 1]) - t0;
        DpLanes q;
        {
            const bool on = (lane >> 3) < n;
            const int tg = t0 + (on ? (lane >> 3) : 0);
            const int rd = a.t.read_idx[tg], uo = a.t.unit_off[tg];
            const long long wo = a.t.b.woff[rd];
            q.pk = a.t.b.packed + wo; q.wlim = a.packed_words - wo;
            q.base = a.t.qs[tg]; q.rows = on ? a.t.qe[tg] - q.base + 1 : 0; q.U = on ? a.t.unit_off[tg + 1] - uo : 0;
            q.unit = a.t.units + uo;
        }
        const int maxrows = uni(wave_max_i32(q.rows)), umax = uni(wave_max_i32(q.U));
        const int C = (umax + 7) >> 3;
        int best[2][3];
        st_fwd2p_oct(C, q, cells, maxrows, best);
        wave_sync_mem();
        const int bestl = st_oct_best_lanes(best);
#pragma unroll 1
        for (int g = 0; g < n; g++) {
            const int tg = t0 + g;
            const int rd = uni(a.t.read_idx[tg]), qs = uni(a.t.qs[tg]), U = uni(a.t.unit_off[tg + 1]) - uni(a.t.unit_off[tg]);
            for (int p = 0; p < 2; p++) {
                const int bk[3] = { lane_val(bestl, 8 * g + 3 * p), lane_val(bestl, 8 * g + 3 * p + 1), lane_val(bestl, 8 * g + 3 * p + 2) };
                DpRes o;
                dpt_traceback<1>(a, a.t.b.packed + uni64(a.t.b.woff[rd]), qs, U, cells + (size_t)g * DPQ_DP_BYTES_G(8, C, maxrows), p, DPQ_ROW_BYTES_G(8, C), bk, o, s_cnt);
                dpt_store(a, tg, p, qs, U, o);
                loop_join();
            }
            loop_join();
        }
        wave_sync_mem();
        loop_join();
    }
    wc_flush(s_cnt, a.t.counters);
}

// MTR_TEST_PASS_FOUR1P, MTR_TEST_PASS_OCT1P: a pass of mtr_k_revise_quads at the widest member's width, then each member's counting traceback
__global__ __launch_bounds__(64, MTR_WAVES_PER_SIMD) void mtr_k_dp_test_rev(DpPassArgs a)
{
    __shared__ unsigned long long s_cnt[CNT_N];
    if (lane_id() < CNT_N) s_cnt[lane_id()] = 0ull;
    uint8_t *cells = a.t.scratch + (size_t)blockIdx.x * a.t.scratch_per_wave;
    for (;;) {
        const int grp = next_work_item(a.t.work_counter);
        if (grp >= a.n_groups) break;
        const int t0 = uni(a.group_off[grp]), n = uni(a.group_off[grp + 1]) - t0;
        DpOct q; q.n = n;
        int maxrows = 0, maxU = 0;
#pragma unroll 1
        for (int g = 0; g < RQ_SLOTS; g++) { q.pk[g] = a.t.b.packed; q.wlim[g] = 1; q.base[g] = 0; q.rows[g] = 0; q.U[g] = 0; q.unit[g] = cells; q.G[g] = 1; q.MM[g] = 1; q.D[g] = 1; }
#pragma unroll 1
        for (int k = 0; k < n; k++) {
            const int tg = t0 + k;
            const int rd = uni(a.t.read_idx[tg]), uo = uni(a.t.unit_off[tg]);
            q.pk[k] = a.t.b.packed + uni64(a.t.b.woff[rd]); q.wlim[k] = a.packed_words - uni64(a.t.b.woff[rd]);
            q.base[k] = uni(a.t.qs[tg]); q.rows[k] = uni(a.t.qe[tg]) - q.base[k] + 1;
            q.U[k] = uni(a.t.unit_off[tg + 1]) - uo; q.unit[k] = a.t.units + uo;
            q.G[k] = uni(a.t.gain[tg]); q.MM[k] = uni(a.t.mism[tg]); q.D[k] = uni(a.t.indel[tg]);
            maxrows = q.rows[k] > maxrows ? q.rows[k] : maxrows; maxU = q.U[k] > maxU ? q.U[k] : maxU;
        }
        const int Cq = DPQ_COLS(maxU);
        int best[RQ_SLOTS][3];
        for (int g = 0; g < RQ_SLOTS; g++) { best[g][0] = 0; best[g][1] = 0; best[g][2] = 0; }
        if (a.pass == MTR_TEST_PASS_FOUR1P) st_fwd1p_four(Cq, q, cells, maxrows, best); else st_fwd1p_any(Cq, q, cells, maxrows, best);
        wave_sync_mem();
#pragma unroll 1
        for (int k = 0; k < n; k++) {
            int bk[3] = { best[0][0], best[0][1], best[0][2] };
#pragma unroll
            for (int h = 1; h < RQ_SLOTS; h++) if (k == h) { bk[0] = best[h][0]; bk[1] = best[h][1]; bk[2] = best[h][2]; }
            const int tg = t0 + k;
            const int rd = uni(a.t.read_idx[tg]), qs = uni(a.t.qs[tg]), U = uni(a.t.unit_off[tg + 1]) - uni(a.t.unit_off[tg]);
            DpRes o;
            dpt_traceback<3>(a, a.t.b.packed + uni64(a.t.b.woff[rd]), qs, U, cells + (size_t)k * DPQP_DP_BYTES(Cq, maxrows), 0, DPQ_ROW_BYTES(Cq), bk, o, s_cnt);
            dpt_store(a, tg, 0, qs, U, o);
            loop_join();
        }
        wave_sync_mem();
        loop_join();
    }
    wc_flush(s_cnt, a.t.counters);
}

// ---- polish_repeat alone (mtr_test_polish): a task per work item through polish(), as the per-read kernel calls it ------------------------
struct PolishTestArgs {
    K2Args a;                      // the batch, the narrow scratch layout (no cells), counters and status
    int32_t n_tasks;
    const int32_t *read_idx, *rep_start, *rep_end, *k;
    const uint8_t *units; const int32_t *scores, *unit_off;      // unit codes 0..3 and node frequencies, concatenated
    uint8_t *out_units; int32_t *out_len;                         // task t's polished unit at MTRC_MAX_PERIOD * t
};
__global__ __launch_bounds__(64, MTR_LAT_WAVES_PER_SIMD) void mtr_k_polish_test(PolishTestArgs p)
{
    __shared__ __attribute__((aligned(16))) int s_arena[MTR_ARENA_INTS];
    __shared__ unsigned long long s_cnt[CNT_N];
    int *s_keys = s_arena, *s_seeds = s_arena + K2_TAB_CAP, *s_stage = s_seeds + MTRC_MAX_SEEDS + 4;
    const int lane = lane_id();
    if (lane < CNT_N) s_cnt[lane] = 0ull;
    K2Ctx c;
    c.a = &p.a; c.wc = s_cnt;
    c.sc = p.a.scratch + (size_t)blockIdx.x * p.a.scratch_per_wave;
    c.y = k2_layout(p.a.Lmax, p.a.cells_cap);
    c.lds_keys = (lds_int *)s_keys; c.seeds = (lds_int *)s_seeds; c.stage = (lds_int *)s_stage;
    c.ties = (int *)(c.sc + c.y.ties); c.fresh = c.ties + MTRC_MAX_TIEBREAKS;
    c.memo_n = 0; c.memo_qs = c.memo_qe = -1; c.memo_U = 0; c.rmemo_n = 0;
    for (;;) {
        const int t = next_work_item(p.a.work_counter);
        if (t >= p.n_tasks) break;
        st_member_ctx(c, p.a, uni(p.read_idx[t]));
        const int uo = uni(p.unit_off[t]), U = uni(p.unit_off[t + 1]) - uo;
        RR r; rr_clear(r);
        r.rep_start = uni(p.rep_start[t]); r.rep_end = uni(p.rep_end[t]); r.kmer = uni(p.k[t]); r.period = U;
        uint8_t *ub = slot_unit(c, 1);
        slot_load_candidate(ub, slot_score(c, 1), p.units + uo, p.scores + uo, U);
        wave_sync_mem();
        polish(c, r, 1);
#pragma unroll 1
        for (int q = lane; q < r.period; q += 64) p.out_units[(size_t)t * MTRC_MAX_PERIOD + q] = ub[q];
        if (lane == 0) p.out_len[t] = r.period;
        wave_sync_mem();                                   // the next task loads over slot 1
        loop_join();
    }
    wc_flush(s_cnt, p.a.counters);
}

// ---- revise_representative_unit alone (mtr_test_revise, MTR_TEST_REVISE_WAVE): a GROUP of tasks per work item through revise(), one after the other on one
// wavefront, as k2_range_select runs the k of a range: the round memo starts empty with the group (c.rmemo_n = 0) and lives across its tasks.  The arena and
// the launch bounds are mtr_k_revise's.  (MTR_TEST_REVISE_SLOTS has no kernel here: the host launches mtr_k_revise_quads itself, test_entries.hip.inc.)
struct ReviseTestArgs {
    K2Args a;                      // the batch, the full scratch layout (cells included), counters and status
    int32_t n_groups;
    const int32_t *group_off, *read_idx, *rr;                    // group g = tasks group_off[g] .. group_off[g + 1]; rr: 13 integers per task in RR's order
    const uint8_t *units; const int32_t *scores, *unit_off;      // unit codes 0..3 and node frequencies, concatenated
    int32_t *out_rr; uint8_t *out_units;                          // task t's record (13 integers) and unit (at MTRC_MAX_PERIOD * t)
};
__global__ __launch_bounds__(64, MTR_WAVES_PER_SIMD) void mtr_k_revise_test(ReviseTestArgs p)
{
    __shared__ __attribute__((aligned(16))) int s_arena[MTR_ARENA_INTS];
    __shared__ unsigned long long s_cnt[CNT_N];
    int *s_keys = s_arena, *s_seeds = s_arena + K2_TAB_CAP, *s_stage = s_seeds + MTRC_MAX_SEEDS + 4;
    const int lane = lane_id();
    if (lane < CNT_N) s_cnt[lane] = 0ull;
    K2Ctx c;
    c.a = &p.a; c.wc = s_cnt;
    c.sc = p.a.scratch + (size_t)blockIdx.x * p.a.scratch_per_wave;
    c.y = k2_layout(p.a.Lmax, p.a.cells_cap);
    c.lds_keys = (lds_int *)s_keys; c.seeds = (lds_int *)s_seeds; c.stage = (lds_int *)s_stage;
    c.ties = (int *)(c.sc + c.y.ties); c.fresh = c.ties + MTRC_MAX_TIEBREAKS;
    for (;;) {
        const int grp = next_work_item(p.a.work_counter);
        if (grp >= p.n_groups) break;
        const int t0 = uni(p.group_off[grp]), t1 = uni(p.group_off[grp + 1]);
        c.memo_n = 0; c.memo_qs = c.memo_qe = -1; c.memo_U = 0; c.rmemo_n = 0;
#pragma unroll 1
        for (int t = t0; t < t1; t++) {
            st_member_ctx(c, p.a, uni(p.read_idx[t]));
            const int uo = uni(p.unit_off[t]), U = uni(p.unit_off[t + 1]) - uo;
            RR cur; st_rr_load(p.rr + (size_t)t * 13, cur);
            uint8_t *ub = slot_unit(c, 1);
            slot_load_candidate(ub, slot_score(c, 1), p.units + uo, p.scores + uo, U);
            wave_sync_mem();
            revise(c, cur);
            if (lane == 0) {
                int32_t *o = p.out_rr + (size_t)t * 13;
                o[0] = cur.rep_start; o[1] = cur.rep_end; o[2] = cur.repeat_len; o[3] = cur.period; o[4] = cur.copies; o[5] = cur.mat; o[6] = cur.mis;
                o[7] = cur.ins; o[8] = cur.del; o[9] = cur.kmer; o[10] = cur.G; o[11] = cur.MM; o[12] = cur.D;
            }
#pragma unroll 1
            for (int q = lane; q < cur.period && q < MTRC_MAX_PERIOD; q += 64) p.out_units[(size_t)t * MTRC_MAX_PERIOD + q] = ub[q];
            wave_sync_mem();                               // the next task loads over slot 1
            loop_join();
        }
        loop_join();
    }
    wc_flush(s_cnt, p.a.counters);
}
