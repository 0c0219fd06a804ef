// window_edits.hip.inc — the edits of windows in device memory (mtr_window_edits_device).  The definition is include/mtr_hip.h's ("window edits");
// the rows with their decisions kept and the walk back are window_edits.h, shared with the host.  The checks, the keys and the task list are the
// window structure's own kernels (mtr_k_ws_check, mtr_k_ws_bases, mtr_k_ws_tasks) on this call's buffers: the same bins, the same length classes.
// A GROUP is 64 consecutive tasks of one bin - one wavefront in every kernel here, a task the same lane in all of them.  Its stored decisions are
// one slot of the transient buffer, [row][word][lane]: the 64 lanes step through the rows in lockstep, so a row's word is one contiguous 256-byte
// line of stores; the slot has the rows of the group's longest window, and the host lays the slots of a ROUND side by side (WeArgs::gslot).
//   mtr_k_we_groups      one wavefront per group: its rows (the longest window's n + 1)
//   mtr_k_we_rows<UB, WIDE>  THE HOT PATH, one window per lane: we_rows - ws_rows' cells with each row's decisions stored - the end's carried
//                        fields and which column is the end
//   mtr_k_we_count       one window per lane: the walk back that counts the edits and, from the steps alone, copies, matches and entries; a window
//                        whose walk does not reproduce what the rows carried forward is left in the state (the smallest)
//   mtr_k_we_emit        one window per lane, after the offset scan (mtr_k_scan_offsets): the walk back once more, every edit written at its
//                        final place, the last first
//   mtr_k_we_output      one lane per window: seg from the WALK's counts, score, skipped (zeros for an empty or skipped window)
// Every result is written with ordinary vector stores.
#pragma once
#include "window_structure.hip.inc"
#include "window_edits.h"

struct WeArgs {
    WsArgs ws;                                                          // the columns, the structures, key, tasks, raw (what the rows carried), the scores
    unsigned bin_first[WS_BINS + 1], grp_first[WS_BINS + 1];            // a bin's tasks and its groups: group g of bin b = tasks bin_first[b] + 64 (g - grp_first[b]) ..
    int32_t *grows;                                                     // [groups] the rows of a group's slot
    const int64_t *gslot;                                               // [groups] where the slot begins in `scratch`, in words
    uint32_t *scratch;
    int32_t *end_id, *n_edits;                                          // [N] each; n_edits zeroed per call
    WeCount *cnt;                                                       // [N] the walk's counts
    const int64_t *off;                                                 // [N + 1]
    int32_t *edits;
    unsigned long long *differs;                                        // the smallest window whose walk is not its rows' path (~0: none)
    int32_t *seg, *score; uint8_t *skipped;                             // the call's own
};

// the task of this lane in group g, or false beyond the bin's end
DEVINL bool we_task(const WeArgs &a, unsigned g, unsigned &task)
{
    unsigned t0 = a.bin_first[0], t1 = a.bin_first[1], g0 = 0;
#pragma unroll
    for (int b = 1; b < WS_BINS; b++) if (g >= a.grp_first[b]) { t0 = a.bin_first[b]; t1 = a.bin_first[b + 1]; g0 = a.grp_first[b]; }
    task = t0 + (g - g0) * 64u + (unsigned)lane_id();
    return task < t1;
}

__global__ __launch_bounds__(64) void mtr_k_we_groups(WeArgs a)
{
    const unsigned g = blockIdx.x;
    unsigned task;
    int n = 0;
    if (we_task(a, g, task)) { const int32_t x = a.ws.tasks[task]; n = (int)(a.ws.win_off[x + 1] - a.ws.win_off[x]); }
    const int rows = wave_max_i32(n) + 1;
    if (lane_id() == 0) a.grows[g] = rows;
}

// <32, narrow> and <16, wide> keep the previous row in LDS - column c of a lane at c * 64 + lane, no bank conflict - and do not unroll the loops over
// the columns (WeRowMem): unrolled over register arrays they take more than 256 registers, and with the row's stores in the loop those two kernels
// computed wrong rows on the device (DESIGN.md 7i-16).  The other three are ws_rows' form: register arrays, unrolled.
template <int UB, bool WIDE>
__global__ __launch_bounds__(64, UB == 8 && !WIDE ? 4 : 2) void mtr_k_we_rows(WeArgs a, unsigned g_first)
{
    typedef typename WsCnt<WIDE>::type P;
    constexpr bool MEM = UB == 32 || (UB == 16 && WIDE);
    const unsigned g = g_first + blockIdx.x;
    unsigned task;
    if (!we_task(a, g, task)) return;
    const int32_t x = a.ws.tasks[task];
    const WsStruct st = a.ws.structs[a.ws.win_struct[x]];
    const int64_t o0 = a.ws.win_off[x];
    const int n = (int)(a.ws.win_off[x + 1] - o0);
    if (st.W > UB || (!WIDE && st.S > 2) || n < 1 || n > WS_MAX_WINDOW || n >= a.grows[g]) return;      // (nothing else reaches here: the bins are the check kernel's, the rows the group's)
    const uint8_t *at = a.ws.win_bases + o0;
    const int r = (int)((uintptr_t)at & 7);
    const uint64_t *wp = (const uint64_t *)(at - r);
    constexpr int NW = UB <= 8 ? 1 : UB <= 16 ? 2 : 3;
    uint32_t *slot = a.scratch + a.gslot[g] + lane_id();
    int end_id = WE_START;
    const auto ld = [wp](int k) { return wp[k]; };
    const auto sink = [slot](int i, const WeRow &rec) {
#pragma unroll
        for (int k = 0; k < NW; k++) slot[((size_t)i * NW + k) * 64] = we_pack(UB, rec, k);
    };
    if constexpr (MEM) {
        __shared__ int sH[UB * 64];
        __shared__ P sE[UB * 64], sC[UB * 64], sM[UB * 64];
        WeRowMem<P> row = { sH + lane_id(), sE + lane_id(), sC + lane_id(), sM + lane_id(), 64 };
        a.ws.raw[x] = we_rows_in<UB, WIDE>(row, ld, sink, r, n, st, a.ws.G, a.ws.MM, a.ws.D, end_id);
    } else {
        a.ws.raw[x] = we_rows<UB, WIDE>(ld, sink, r, n, st, a.ws.G, a.ws.MM, a.ws.D, end_id);
    }
    a.end_id[x] = end_id;
}

template <bool EMIT>
DEVINL void we_walk_lane(const WeArgs &a, unsigned g)
{
    unsigned task;
    if (!we_task(a, g, task)) return;
    const int32_t x = a.ws.tasks[task];
    const WsStruct st = a.ws.structs[a.ws.win_struct[x]];
    const int64_t o0 = a.ws.win_off[x];
    const int n = (int)(a.ws.win_off[x + 1] - o0);
    if (n < 1 || n > WS_MAX_WINDOW || n >= a.grows[g]) return;
    const int UB = ws_bucket(st.W), NW = we_row_words(UB);
    const uint32_t *slot = a.scratch + a.gslot[g] + lane_id();
    const auto row = [slot, UB, NW](int i) {
        const uint32_t *p = slot + (size_t)i * NW * 64;
        const uint32_t w0 = p[0], w1 = NW > 1 ? p[64] : 0u, w2 = NW > 2 ? p[128] : 0u;
        return we_unpack(UB, w0, w1, w2);
    };
    const uint8_t *y = a.ws.win_bases + o0;
    const auto base = [y](int p) { return y[p]; };
    if (!EMIT) {
        const WeCount k = we_walk<false>(row, base, n, st, a.end_id[x], 0ull, 0, nullptr);
        const WsRaw raw = a.ws.raw[x];
        if (k.bad || k.entry != raw.entry || k.copies != raw.copies || k.matches != raw.matches) atomicMin(a.differs, (unsigned long long)x);
        a.cnt[x] = k; a.n_edits[x] = k.bad ? 0 : k.edits;
    } else {
        const WeCount c = a.cnt[x];
        if (c.bad) return;
        const WeCount k = we_walk<true>(row, base, n, st, a.end_id[x], c.copies, c.edits, a.edits + WE_FIELDS * a.off[x + 1]);
        if (k.bad || k.edits != c.edits) atomicMin(a.differs, (unsigned long long)x);
    }
}
__global__ __launch_bounds__(64) void mtr_k_we_count(WeArgs a, unsigned g_first) { we_walk_lane<false>(a, g_first + blockIdx.x); }
__global__ __launch_bounds__(64) void mtr_k_we_emit(WeArgs a, unsigned g_first) { we_walk_lane<true>(a, g_first + blockIdx.x); }

__global__ __launch_bounds__(WS_BLOCK) void mtr_k_we_output(WeArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * WS_BLOCK + threadIdx.x;
    if (x >= a.ws.N) return;
    const int64_t n = a.ws.win_off[x + 1] - a.ws.win_off[x];
    int32_t *seg = a.seg + 4 * WS_MAX_SEGMENTS * x;
    int32_t score = 0;
    if (a.ws.key[x] >= 0) {
        const WeCount k = a.cnt[x];
        const WsRaw raw = { a.ws.raw[x].score, 0u, k.entry, k.copies, k.matches };
        ws_spans(raw, (int)n, a.ws.structs[a.ws.win_struct[x]].S, seg);
        score = raw.score;
    } else {
        for (int k = 0; k < 4 * WS_MAX_SEGMENTS; k++) seg[k] = 0;
    }
    a.score[x] = score; a.skipped[x] = n > WS_MAX_WINDOW ? 1 : 0;
}
