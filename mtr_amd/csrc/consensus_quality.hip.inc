// consensus_quality.hip.inc — the quality-weighted allele consensus (mtr_allele_consensus_quality_device).  The definition is include/mtr_hip.h's
// ("quality-weighted allele consensus"); the lists are consensus.hip.inc's kernels as they are (check, members, alleles, tasks), the alignment is
// its band, cell and schedule (banded_align.h), and only the votes differ: the walk adds a base's weight instead of 1 (baq_walk), a position's
// table has BAQ_TAB counters, and the emission weighs the backbone's own votes too (baq_emit).  Every result is an exact integer: the votes are
// integer atomic adds, whose order reaches no sum, and the host refuses a call whose sums could leave int32.
//   mtr_k_cq_align<CPL>  one alignment per wavefront: mtr_k_cons_align's fill - the same anti-diagonal steps, the one DPP shift per step, the
//                        directions 16 steps a dword in the wavefront's scratch -, then the weighted walk by lane 0: per step one byte load of the
//                        quality and one clamp more than the unweighted walk, per column one more atomic (end)
//   mtr_k_cq_emit<W>     one workgroup per allele: per position its symbols (baq_emit), a scan, and - W = 1 - the writes; W = 0 gives the lengths
#pragma once
#include "consensus.hip.inc"

struct ConsQArgs { ConsArgs c; const uint8_t *win_qual; int32_t qual_cap; };       // win_qual [n_bases]: the Phred value of win_bases' base

template <int CPL>
__global__ __launch_bounds__(64) void mtr_k_cq_align(ConsQArgs q, int bucket, unsigned n_tasks, uint32_t *scratch, int64_t words_per_wave)
{
    const ConsArgs &a = q.c;
    const int lane = lane_id();
    uint32_t *dirs = scratch + (int64_t)blockIdx.x * words_per_wave;
    for (unsigned t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const int4 task = a.tasks[(int64_t)bucket * a.S + t];
        const int A = uni(task.x), row = uni(task.y), bb = uni(task.z);
        const int64_t wo = uni64(a.win_off[row]), bo = uni64(a.win_off[bb]);
        const int32_t n = uni((int)(a.win_off[row + 1] - wo)), m = uni((int)(a.win_off[bb + 1] - bo));
        const uint8_t *W = a.win_bases + wo, *B = a.win_bases + bo;
        const BaBand band = ba_band(n, m, a.band_extra);
        if (ba_dir_words(n, m, CPL) <= words_per_wave && ba_width(band) <= 128 * CPL) {        // (the host sized both: nothing is stored past them)
            int32_t E[CPL], O[CPL]; uint32_t acc[CPL];
#pragma unroll
            for (int k = 0; k < CPL; k++) { E[k] = O[k] = BA_INF; acc[k] = 0u; }
            for (int32_t s = 0; s <= n + m; s++) {
                const int sh = 2 * (s & 15);
                if (((s - band.dlo) & 1) == 0) {
                    const int32_t below = shift_up1(O[CPL - 1], BA_INF);
#pragma unroll
                    for (int k = 0; k < CPL; k++) {
                        int dir;
                        E[k] = ba_step_cell(s, 2 * (lane * CPL + k), n, m, band, E[k], O[k], k > 0 ? O[k > 0 ? k - 1 : 0] : below, W, B, dir);
                        acc[k] |= (uint32_t)dir << sh;
                    }
                } else {
                    const int32_t above = shift_down1(E[0], BA_INF);
#pragma unroll
                    for (int k = 0; k < CPL; k++) {
                        int dir;
                        O[k] = ba_step_cell(s, 2 * (lane * CPL + k) + 1, n, m, band, O[k], k + 1 < CPL ? E[k + 1 < CPL ? k + 1 : 0] : above, E[k], W, B, dir);
                        acc[k] |= (uint32_t)dir << sh;
                    }
                }
                if (sh == 30 || s == n + m) {
#pragma unroll
                    for (int k = 0; k < CPL; k++) { dirs[((int64_t)(s >> 4) * CPL + k) * 64 + lane] = acc[k]; acc[k] = 0u; }
                }
            }
            wave_sync_mem();
            if (lane == 0) {
                int32_t *tab = a.tab + a.tab_off[A] * BAQ_TAB;
                const int32_t dlo = band.dlo;
                baq_walk(n, m, W, q.win_qual + wo, q.qual_cap, [=](int32_t i, int32_t j) { return ba_dir_at(dirs, i, j, dlo, CPL); },
                         [=](int64_t x, int32_t w) { atomicAdd(tab + x, w); });
            }
            wave_sync_mem();                                            // (the walk has read the directions before the next task's overwrite them)
        }
        loop_join();
    }
}

template <int WRITE>
__global__ __launch_bounds__(CO_BLOCK) void mtr_k_cq_emit(ConsQArgs q)
{
    __shared__ int32_t part[CO_BLOCK / 64];
    const ConsArgs &a = q.c;
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (int64_t A = blockIdx.x; A < 2 * (int64_t)a.n_loci; A += gridDim.x) {
        const int32_t row = a.bb_row[A], m = a.bb_len[A];
        int64_t before = 0;
        if (row >= 0) {
            const uint8_t *B = a.win_bases + a.win_off[row], *QB = q.win_qual + a.win_off[row];
            const int32_t *tab = a.tab + a.tab_off[A] * BAQ_TAB;
            for (int32_t c = 0; c <= m; c += CO_BLOCK) {
                const int32_t j = c + tid;
                uint8_t sym[1 + BA_INS_SLOTS]; int32_t vt[1 + BA_INS_SLOTS];
                int em = 0;
                if (j <= m) em = baq_emit(tab + (int64_t)j * BAQ_TAB, j, j >= 1 ? B[j - 1] : 0, j >= 1 ? baq_weight(QB[j - 1], q.qual_cap) : 0, baq_gap(QB, m, j, q.qual_cap), sym, vt);
                const int has_base = em & 1, n_ins = em >> 1, cnt = has_base + n_ins;
                int inc = cnt;
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
                __syncthreads();
                if (lane == 63) part[wave] = inc;
                __syncthreads();
                int total = 0;
                for (int w = 0; w < CO_BLOCK / 64; w++) { const int s = part[w]; if (w < wave) inc += s; total += s; }
                if (WRITE) {
                    const int64_t at = a.cons_off[A] + before + inc - cnt;
#pragma unroll
                    for (int k = 0; k < 1 + BA_INS_SLOTS; k++)
                        if (k == 0 ? has_base : k <= n_ins) { const int64_t to = at + (k == 0 ? 0 : has_base + k - 1); a.bases[to] = sym[k]; a.votes[to] = vt[k]; }
                }
                before += total;
            }
        }
        if (!WRITE && tid == 0) a.cons_len[A] = (int32_t)before;
    }
}
