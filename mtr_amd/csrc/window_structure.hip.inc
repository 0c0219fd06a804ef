// window_structure.hip.inc — the motif structure of windows in device memory (mtr_window_structure_device).  The definition is include/mtr_hip.h's
// ("window structure"); the row body, the carried fields and the spans are window_structure.h, shared with the host.  Every output but ratio is an
// exact integer; the task lists are filled by atomics whose order decides which lane runs a window and reaches no result.
//   mtr_k_ws_check       one lane per window: win_off ascending from 0 to n_bases, win_struct inside the structures (the smallest bad window is left
//                        in the state); a window that is neither empty nor skipped counts into its key = bin * 16 + length class, one add per key
//                        and wavefront
//   mtr_k_ws_bases       one lane per aligned 8 bytes of win_bases: the smallest position of a code above 3
//   mtr_k_ws_tasks       one lane per window: its slot in the task list, the keys side by side - bin (column bucket, counter width), then length
//                        class, so that the 64 lanes of a wavefront run windows of similar length
//   mtr_k_ws_lanes<UB, WIDE>  THE HOT PATH, one window per lane: ws_rows with the lane's own structure, the previous row in register arrays, the
//                        window 8 aligned bytes a load; nothing is stored per cell - the end's carried fields are the result
//   mtr_k_ws_output      one lane per window: the carried entries become spans, the columns of dst are written (zeros for an empty or skipped window)
#pragma once
#include "device_util.hip.inc"
#include "window_structure.h"

#define WS_BLOCK 256
#define WS_BAD 3                    // uint64 each, ~0: none.  0 win_off, 1 win_struct, 2 a base code
#define WS_BINS 5                   // <8, narrow>, <16, narrow>, <32, narrow>, <8, wide>, <16, wide>
#define WS_CLASSES 16               // the length class of n in 1 .. WS_MAX_WINDOW: the bits of n
#define WS_KEYS (WS_BINS * WS_CLASSES)

struct WsArgs {
    const int64_t *win_off; const uint8_t *win_bases; const int32_t *win_struct; int64_t N, n_bases; int32_t n_structs;
    const WsStruct *structs;                                            // [n_structs]
    unsigned *count, *cursor;                                           // [WS_KEYS] each, zeroed per call
    int32_t *key, *tasks;                                               // [N] each: a window's key (-1: no DP), the windows in task order
    WsRaw *raw;                                                         // [N]
    unsigned long long *bad;
    int32_t G, MM, D;
    int32_t *seg, *score; float *ratio; uint8_t *skipped;               // the caller's
};

DEVINL int ws_bin(int W, int S) { return (S > 2 ? 3 : 0) + (W <= 8 ? 0 : W <= 16 ? 1 : 2); }

__global__ __launch_bounds__(WS_BLOCK) void mtr_k_ws_check(WsArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * WS_BLOCK + threadIdx.x;
    if (a.N == 0) { if (x == 0 && (a.win_off[0] != 0 || a.n_bases != 0)) atomicMin(&a.bad[0], 0ull); return; }
    int32_t key = -1;
    if (x < a.N) {
        const int64_t o0 = a.win_off[x], o1 = a.win_off[x + 1];
        const int32_t k = a.win_struct[x];
        const bool off_ok = o0 >= 0 && o1 >= o0 && o1 <= a.n_bases && (x > 0 || o0 == 0) && (x < a.N - 1 || o1 == a.n_bases), k_ok = k >= 0 && k < a.n_structs;
        if (!off_ok) atomicMin(&a.bad[0], (unsigned long long)x);
        if (!k_ok) atomicMin(&a.bad[1], (unsigned long long)x);
        if (off_ok && k_ok && o1 > o0 && o1 - o0 <= WS_MAX_WINDOW) key = ws_bin(a.structs[k].W, a.structs[k].S) * WS_CLASSES + (32 - __clz((int)(o1 - o0)));
        a.key[x] = key;
    }
    // one add per key the wavefront holds (a batch of one locus is one key: its windows' adds would queue up on one address)
    for (unsigned long long left = __ballot(key >= 0); left;) {
        const int leader = first_lane(left), k = lane_val(key, leader);
        const unsigned long long same = __ballot(key == k);
        if (lane_id() == leader) atomicAdd(&a.count[k], (unsigned)__popcll(same));
        left &= ~same;
    }
}

// words: the aligned 8-byte words that hold a byte of win_bases; an aligned word lies inside the page of each of its bytes
__global__ __launch_bounds__(WS_BLOCK) void mtr_k_ws_bases(const uint8_t *bases, int64_t n_bases, int64_t words, unsigned long long *bad)
{
    const int r = (int)((uintptr_t)bases & 7);
    const uint64_t *wp = (const uint64_t *)(bases - r);
    for (int64_t k = (int64_t)blockIdx.x * WS_BLOCK + threadIdx.x; k < words; k += (int64_t)gridDim.x * WS_BLOCK) {
        const uint64_t w = wp[k];
        if ((w & 0xfcfcfcfcfcfcfcfcull) == 0) continue;
        for (int b = 0; b < 8; b++) {
            const int64_t p = 8 * k + b - r;
            if (p >= 0 && p < n_bases && ((w >> (8 * b)) & 0xfcu)) { atomicMin(&bad[2], (unsigned long long)p); break; }
        }
    }
}

__global__ __launch_bounds__(WS_BLOCK) void mtr_k_ws_tasks(WsArgs a)
{
    __shared__ unsigned start[WS_KEYS];
    if (threadIdx.x < WS_KEYS) { unsigned s = 0; for (unsigned k = 0; k < threadIdx.x; k++) s += a.count[k]; start[threadIdx.x] = s; }
    __syncthreads();
    const int64_t x = (int64_t)blockIdx.x * WS_BLOCK + threadIdx.x;
    const int32_t key = x < a.N ? a.key[x] : -1;
    for (unsigned long long left = __ballot(key >= 0); left;) {          // one add per key of the wavefront, as in the check
        const int leader = first_lane(left), k = lane_val(key, leader);
        const unsigned long long same = __ballot(key == k);
        unsigned base = 0;
        if (lane_id() == leader) base = start[k] + atomicAdd(&a.cursor[k], (unsigned)__popcll(same));
        const unsigned slot = (unsigned)bcast((int)base, leader) + (unsigned)mbcnt(same);
        if (key == k && (int64_t)slot < a.N) a.tasks[slot] = (int32_t)x;
        left &= ~same;
    }
}

template <int UB, bool WIDE>
__global__ __launch_bounds__(64) void mtr_k_ws_lanes(WsArgs a, unsigned first, unsigned n_tasks)
{
    const unsigned t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n_tasks) return;
    const int32_t x = a.tasks[first + t];
    const WsStruct st = a.structs[a.win_struct[x]];
    const int64_t o0 = a.win_off[x];
    const int n = (int)(a.win_off[x + 1] - o0);
    if (st.W > UB || (!WIDE && st.S > 2) || n < 1 || n > WS_MAX_WINDOW) return;         // (the bins are the check kernel's: nothing else reaches here)
    const uint8_t *at = a.win_bases + o0;
    const int r = (int)((uintptr_t)at & 7);
    const uint64_t *wp = (const uint64_t *)(at - r);                   // word k holds y[8k - r .. 8k - r + 8): each asked for holds a byte of the window
    a.raw[x] = ws_rows<UB, WIDE>([wp](int k) { return wp[k]; }, r, n, st, a.G, a.MM, a.D);
}

__global__ __launch_bounds__(WS_BLOCK) void mtr_k_ws_output(WsArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * WS_BLOCK + threadIdx.x;
    if (x >= a.N) return;
    const int64_t n = a.win_off[x + 1] - a.win_off[x];
    int32_t *seg = a.seg + 4 * WS_MAX_SEGMENTS * x;
    int32_t score = 0; float ratio = 0.0f;
    if (a.key[x] >= 0) {
        const WsRaw raw = a.raw[x];
        ws_spans(raw, (int)n, a.structs[a.win_struct[x]].S, seg);
        score = raw.score; ratio = (float)ws_matches(raw) / (float)(int)n;
    } else {
        for (int k = 0; k < 4 * WS_MAX_SEGMENTS; k++) seg[k] = 0;
    }
    a.score[x] = score; a.ratio[x] = ratio; a.skipped[x] = n > WS_MAX_WINDOW ? 1 : 0;
}
