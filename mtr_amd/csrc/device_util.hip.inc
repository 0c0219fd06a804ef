// device_util.hip.inc — wave64 helpers for the gfx950 kernels.  One wavefront works on one read; every
// "scalar" below is kept wave-uniform, lanes carry the data-parallel index.
#pragma once
#include <hip/hip_runtime.h>
#include "mtr_common.h"
#include "walk_screen.h"

#define DEVINL __device__ __forceinline__

typedef __attribute__((address_space(3))) int lds_int;   // forces ds_* addressing (a generic int* becomes flat_*)
typedef __attribute__((address_space(3))) unsigned char lds_u8;

DEVINL int lane_id() { return (int)(threadIdx.x & 63u); }
// The reference's WrapDPsize (mTR.h:51, wrap_around_DP.c:95-99 / :259-262) as the kernels test it.  A device variable, not the literal: no input of
// at most 833 333 bases is known to reach 2e8 cells, so the GPU suite lowers the limit on both sides (MTR_TEST_WRAP_DP_SIZE, read by mtr_create and by
// the oracle) to make the kernels raise MTR_ERR_DP_TOO_LARGE.  The address is a constant: one scalar load per DP.
__device__ long long mtr_dev_wrap_dp_size = MTRC_WRAP_DP_SIZE;
DEVINL bool dp_size_ok(int U, int rows) { return (size_t)(U + 1) * (size_t)rows + (size_t)U < (size_t)mtr_dev_wrap_dp_size; }
// uni(): tell the compiler that a value is wave-uniform (v_readfirstlane -> SGPR).  hipcc treats every value that
// came out of a vector load, an LDS read, a ds_bpermute shuffle or a loop with a lane-dependent exit as
// divergent, and then keeps the whole dependent "scalar" computation in VGPRs with exec-masked branches
// (the traceback walk compiled to ~75 VALU instructions per step that way, ~30 scalar ones after).
DEVINL int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEVINL long long uni64(long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
DEVINL int bcast(int v, int src) { return __shfl(v, src, 64); }
DEVINL unsigned long long lanemask_lt() { return (1ull << lane_id()) - 1ull; }
DEVINL int mbcnt(unsigned long long m)
{   // number of set bits of m in lanes strictly below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
DEVINL int first_lane(unsigned long long m) { return __ffsll((long long)m) - 1; }

// (2-bit packed reads: base_at, kmer_at - walk_screen.h, shared with the host)

DEVINL unsigned scan_max_u32(unsigned v);
// ---- wave reductions / scans ---------------------------------------------------------------------------
DEVINL int wave_max_i32(int v)
{
    for (int d = 32; d > 0; d >>= 1) { int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}
// wave-uniform value of lane `l` (l wave-uniform): v_readlane_b32, no LDS crossbar round trip
DEVINL int lane_val(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
// v with lane l (wave-uniform; the hardware takes l mod 64) replaced by the wave-uniform val: v_writelane_b32 (hipcc has no builtin for it)
DEVINL int write_lane(int v, int val, int l)
{
    asm("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(val), "s"(l) : "m0");      // (one SGPR on gfx9's constant bus: the lane select goes through M0)
    return v;
}
// two registers at once: lane l mod 64 of a / b becomes va / vb
DEVINL void write_lane2(int &a, int &b, int va, int vb, int l)
{
    // (s_mov, not s_and: an instruction in here that writes SCC would do so behind the compiler's back - it schedules this between a compare and its branch)
    asm("s_mov_b32 m0, %4\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %3, m0" : "+v"(a), "+v"(b) : "s"(va), "s"(vb), "s"(l & 63) : "m0");
}
DEVINL long long lane_val64(long long v, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// maximum over the wave of values >= -1, as a DPP prefix scan + readlane of the last lane
DEVINL int wave_max_i32_dpp(int v) { return lane_val((int)scan_max_u32((unsigned)(v + 1)), 63) - 1; }
DEVINL long long wave_sum_i64(long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// inclusive prefix max of an unsigned key over the 64 lanes, DPP row shifts + row broadcasts
// (the gfx9 scan: row_shr 1,2,4,8, row_bcast15 on rows 1/3, row_bcast31 on rows 2/3).
DEVINL unsigned scan_max_u32(unsigned v)
{
    unsigned t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); v = t > v ? t : v;   // row_shr:1
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); v = t > v ? t : v;   // row_shr:2
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); v = t > v ? t : v;   // row_shr:4
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); v = t > v ? t : v;   // row_shr:8
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); v = t > v ? t : v;   // row_bcast:15
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); v = t > v ? t : v;   // row_bcast:31
    return v;
}
// two independent prefix-max scans in lockstep: the steps of one fill the DPP wait states of the other
DEVINL void scan_max_u32_x2(unsigned &a, unsigned &b)
{
    unsigned s, t;
#define MTR_SCAN_STEP(ctrl, rm) \
    s = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a, ctrl, rm, 0xf, false); \
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b, ctrl, rm, 0xf, false); \
    a = s > a ? s : a; b = t > b ? t : b;
    MTR_SCAN_STEP(0x111, 0xf) MTR_SCAN_STEP(0x112, 0xf) MTR_SCAN_STEP(0x114, 0xf) MTR_SCAN_STEP(0x118, 0xf)
    MTR_SCAN_STEP(0x142, 0xa) MTR_SCAN_STEP(0x143, 0xc)
#undef MTR_SCAN_STEP
}
// the same within each ROW of 16 lanes (four independent scans, four steps): the DPP row shifts never leave a row
DEVINL void scan_max_u32_x2_row16(unsigned &a, unsigned &b)
{
    unsigned s, t;
#define MTR_SCAN_STEP(ctrl) \
    s = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a, ctrl, 0xf, 0xf, false); \
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b, ctrl, 0xf, 0xf, false); \
    a = s > a ? s : a; b = t > b ? t : b;
    MTR_SCAN_STEP(0x111) MTR_SCAN_STEP(0x112) MTR_SCAN_STEP(0x114) MTR_SCAN_STEP(0x118)
#undef MTR_SCAN_STEP
}
// value of the previous lane of the same 16-lane row (the row's first lane receives its own `first`): row_shr:1
DEVINL int row_shift_up1(int v, int first)
{
    return __builtin_amdgcn_update_dpp(first, v, 0x111, 0xf, 0xf, false);
}
// ---- two 16-bit values per register (the two parameter sets of wrap_around_DP side by side) ----------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
DEVINL u16x2 as_pk(unsigned v) { return __builtin_bit_cast(u16x2, v); }
DEVINL unsigned as_u32(u16x2 v) { return __builtin_bit_cast(unsigned, v); }
DEVINL unsigned pk_add(unsigned a, unsigned b) { return as_u32(as_pk(a) + as_pk(b)); }                                   // v_pk_add_u16
DEVINL unsigned pk_sub(unsigned a, unsigned b) { return as_u32(as_pk(a) - as_pk(b)); }                                   // v_pk_sub_u16
DEVINL unsigned pk_sub_sat(unsigned a, unsigned b) { return as_u32(__builtin_elementwise_sub_sat(as_pk(a), as_pk(b))); } // ... clamp: max(0, a-b)
DEVINL unsigned max3_u32(unsigned a, unsigned b, unsigned c) { unsigned r; asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
DEVINL unsigned pk_max(unsigned a, unsigned b) { return as_u32(__builtin_elementwise_max(as_pk(a), as_pk(b))); }         // v_pk_max_u16
DEVINL unsigned pk_min(unsigned a, unsigned b) { return as_u32(__builtin_elementwise_min(as_pk(a), as_pk(b))); }         // v_pk_min_u16
// (a << sh) | b in one instruction (hipcc makes two shifts and a v_or3 of a chain of them)
template <int SH>
DEVINL unsigned lshl_or(unsigned a, unsigned b)
{
    unsigned r;
    asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "n"(SH), "v"(b));
    return r;
}
// min(x, 1) per half = "x != 0" as 0/1.  Written as asm because hipcc turns the generic form into two 16-bit compares,
// two selects and a v_perm (6 instructions instead of 1).
DEVINL unsigned pk_nonzero(unsigned a, unsigned one_pk)
{
    unsigned r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(one_pk));
    return r;
}

// value of lane-1 (lane 0 receives `first`): wave_shr:1
DEVINL int shift_up1(int v, int first)
{
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);
}

// running maximum with the EARLIEST position on ties (strict '>' replaces), inclusive over lanes
DEVINL void scan_max_first(double &v, int &idx)
{
    int lane = lane_id();
    for (int d = 1; d < 64; d <<= 1) {
        double ov = __shfl_up(v, d, 64); int oi = __shfl_up(idx, d, 64);
        if (lane >= d && !(v > ov)) { v = ov; idx = oi; }
    }
}
// running minimum with the earliest position on ties (strict '<' replaces)
DEVINL void scan_min_first(double &v, int &idx)
{
    int lane = lane_id();
    for (int d = 1; d < 64; d <<= 1) {
        double ov = __shfl_up(v, d, 64); int oi = __shfl_up(idx, d, 64);
        if (lane >= d && !(v < ov)) { v = ov; idx = oi; }
    }
}

// next item of a device-wide work queue, wave-uniform.  The empty asm keeps the per-lane value opaque:
// without it hipcc (ROCm 7.2) knows that lanes 1..63 hold the constant 0, folds readfirstlane(0) for
// them, and threads those lanes around the loop's exit test -> they spin forever on item 0
// (observed on gfx950; see DESIGN.md "compiler hazards").
DEVINL int next_work_item(unsigned int *counter)
{
    int t = 0;
    if (lane_id() == 0) t = (int)atomicAdd(counter, 1u);
    asm volatile("" : "+v"(t));
    return __builtin_amdgcn_readfirstlane(t);
}

// A work queue with sub-queues.  ONE counter completes 88 M returning atomics per second on this chip, whatever the number
// of wavefronts that pull from it (tests/dev/atomic_rate.hip: 11.3 ns each) - the 2.2 M (read, range) items of a
// 10 000-read batch through one counter are 25 ms, which WAS the duration of the staged mode's first walk kernel.  Counters
// 256 bytes apart complete side by side (8: 576 M/s, 64: 4.5 G/s).  So a queue is up to WQ_MAX counters; item i belongs to
// sub-queue i % nq; a wavefront starts at sub-queue blockIdx % nq and moves on when one is empty, so every wavefront ends after
// at most nq empty pulls.  nq follows from the number of items (a pure function of it: every wavefront derives the same):
// small batches keep ONE counter, because an empty pull is a memory round trip at the end of every kernel of the chain.
#define WQ_MAX 64
#define WQ_STRIDE 64                 // 32-bit words between two counters
#define WQ_WORDS (WQ_MAX * WQ_STRIDE)
struct Wq { int q, nq, tried; };
DEVINL int wq_count(unsigned n) { return n >= 131072u ? 64 : n >= 32768u ? 16 : n >= 8192u ? 4 : 1; }
DEVINL void wq_init(Wq &w, unsigned n) { w.nq = wq_count(n); w.q = (int)(blockIdx.x & (unsigned)(w.nq - 1)); w.tried = 0; }
// Round 6, built and NOT adopted (-DMTR_WQ_PEEK): a wavefront whose sub-queue is empty LOOKS before it pulls again - one load of all the counters (lane q:
// sub-queue q) says which sub-queues still hold items; it moves to the next of those, or leaves.  Without it every wavefront ends every kernel of the chain with
// one empty pull per sub-queue (64 dependent atomic round trips; the whole duration of mtr_k_rev_share / mtr_k_finish).  [measured, one box, three rounds each]
// the service kernels' wavefront-cycles fall (mtr_k_rev_share 8.0 -> 4.5 G, mtr_k_finish 6.1 -> 3.6 G per launch) and a lone launch is 0.3 ms shorter (43.7
// against 44.0 ms) - and the pipelined step is 0.45 ms LONGER (35.62 against 35.16 ms): what the step is made of is not those kernels' residence time.
// Returns the sub-queue to try next (>= 0), or -1: all empty.
DEVINL int wq_peek_next(unsigned int *base, unsigned n, int nq, int q, unsigned B)
{
    const int lane = lane_id();
    unsigned left = 0u;
    if (lane < nq && (unsigned)lane < n) {
        const unsigned have = (n - (unsigned)lane + (unsigned)nq - 1u) / (unsigned)nq;              // items of sub-queue `lane`: lane, lane + nq, ...
        const unsigned taken = __hip_atomic_load(base + lane * WQ_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        left = taken < have ? have - taken : 0u;
    }
    (void)B;
    const unsigned long long m = __ballot(left != 0u);
    if (m == 0ull) return -1;
    const unsigned long long behind = q < 63 ? m & (~0ull << (q + 1)) : 0ull;                      // the next one in turn, so that the wavefronts spread
    return behind != 0ull ? __builtin_ctzll(behind) : __builtin_ctzll(m);
}
// the next item of a queue of n items, -1 when every sub-queue is empty (every wavefront gets there)
DEVINL int wq_next(unsigned int *base, unsigned n, Wq &w)
{
#ifdef MTR_WQ_PEEK
    for (;;) {
        int t = 0;
        if (lane_id() == 0) t = (int)atomicAdd(base + w.q * WQ_STRIDE, 1u);
        asm volatile("" : "+v"(t));
        const unsigned long long idx = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(t) * (unsigned)w.nq + (unsigned)w.q;
        if (idx < (unsigned long long)n) return (int)idx;
        if (w.nq == 1) return -1;
        const int nx = wq_peek_next(base, n, w.nq, w.q, 1u);
        if (nx < 0) return -1;
        w.q = nx;
        __builtin_amdgcn_wave_barrier();
    }
#else
    int item = -1;
    while (w.tried < w.nq) {
        int t = 0;
        if (lane_id() == 0) t = (int)atomicAdd(base + w.q * WQ_STRIDE, 1u);
        asm volatile("" : "+v"(t));
        const unsigned long long idx = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(t) * (unsigned)w.nq + (unsigned)w.q;
        if (idx < (unsigned long long)n) { item = (int)idx; break; }
        w.q = (w.q + 1) & (w.nq - 1); w.tried++;
        __builtin_amdgcn_wave_barrier();
    }
    return item;
#endif
}

// B consecutive items of one sub-queue with ONE pull: the first item's index (the b-th is that + b * w.nq, valid while < n), -1 when every
// sub-queue is empty.  A work item of the chain starts with a chain of dependent memory round trips (the pull, its record, the read's length and
// offset): pulled four at a time the round trips of four items overlap (k3_staged.hip.inc: mtr_k_walks).
DEVINL long long wq_next_batch(unsigned int *base, unsigned n, Wq &w, unsigned B)
{
#ifndef MTR_WQ_PEEK
    long long item = -1;
    while (w.tried < w.nq) {
        int t = 0;
        if (lane_id() == 0) t = (int)atomicAdd(base + w.q * WQ_STRIDE, B);
        asm volatile("" : "+v"(t));
        const unsigned long long idx = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(t) * (unsigned)w.nq + (unsigned)w.q;
        if (idx < (unsigned long long)n) { item = (long long)idx; break; }
        w.q = (w.q + 1) & (w.nq - 1); w.tried++;
        __builtin_amdgcn_wave_barrier();
    }
    return item;
#endif
    for (;;) {
        int t = 0;
        if (lane_id() == 0) t = (int)atomicAdd(base + w.q * WQ_STRIDE, B);
        asm volatile("" : "+v"(t));
        const unsigned long long idx = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(t) * (unsigned)w.nq + (unsigned)w.q;
        if (idx < (unsigned long long)n) return (long long)idx;
        if (w.nq == 1) return -1;
        const int nx = wq_peek_next(base, n, w.nq, w.q, B);
        if (nx < 0) return -1;
        w.q = nx;
        __builtin_amdgcn_wave_barrier();
    }
}

// Put at the END of a loop body that contains lane-divergent blocks (if (lane == 0) ...) and whose header
// runs cross-lane operations (readfirstlane / ballot / shuffles / DPP).  Without a convergent operation
// in front of the back-edge hipcc (ROCm 7.2) gives the divergent paths their own back-edges, the
// structurizer turns them into nested loops, and lanes 1..63 re-enter the header without lane 0: the
// cross-lane operation then sees a partial wave (mtr_k_dp_test spun forever on gfx950 this way).
DEVINL void loop_join() { __builtin_amdgcn_wave_barrier(); }

DEVINL void count_add(unsigned long long *counters, int which, long long v)
{
    if (lane_id() == 0) atomicAdd(&counters[which], (unsigned long long)v);
}
// Per-wave work counters live in LDS and are flushed with one atomic per counter and read: 25 M global
// atomics on one cache line per launch (the first build) made every wave wait on contended atomics.
DEVINL void wc_add(unsigned long long *wc, int which, long long v)
{
    if (lane_id() == 0) wc[which] += (unsigned long long)v;
}
// phase timers: shader clock (s_memtime) deltas accumulated into the per-wave counters.  Compiled in only with
// -DMTR_PROFILE (mtr_amd/libmtr_hip_prof.so, used by tests/dev/gpu_phase.py): every s_memtime drains the wave's
// outstanding LDS / scalar-memory operations, and the ~40 timer sites run thousands of times per read.
#ifdef MTR_PROFILE
DEVINL unsigned long long clk() { return __builtin_amdgcn_s_memtime(); }
DEVINL void wc_time(unsigned long long *wc, int which, unsigned long long t0) { wc_add(wc, which, (long long)(clk() - t0)); }
#else
DEVINL unsigned long long clk() { return 0ull; }
DEVINL void wc_time(unsigned long long *, int, unsigned long long) {}
#endif
// timers that share a spare counter with a development build's own use of it (-DMTR_PROFILE_WALK_FMT: k2_units.hip.inc walk();
// -DMTR_PROFILE_DP2_CLASS: k3_staged.hip.inc st_quad_run(); -DMTR_PROFILE_POLISH: mtr_k_polish and polish(), k2_units.hip.inc)
#if defined(MTR_PROFILE_WALK_FMT) || defined(MTR_PROFILE_DP2_CLASS) || defined(MTR_PROFILE_POLISH)
#define wc_time_aux(wc, which, t0) do { } while (0)
#else
#define wc_time_aux(wc, which, t0) wc_time(wc, which, t0)
#endif
// -DMTR_PROFILE -DMTR_PROFILE_POLISH (tests/dev/polish_phases.py): the phases of a polish work item, each in a spare counter - 43 queue pull and
// item loads, 44 candidate in, 45 staging and the flag test, 46 table build, 47 the walk, 55 result out
#ifdef MTR_PROFILE_POLISH
#define wc_time_pol(wc, which, t0) wc_time(wc, which, t0)
#else
#define wc_time_pol(wc, which, t0) do { } while (0)
#endif
DEVINL void wc_flush(unsigned long long *wc, unsigned long long *global)
{
    const int lane = lane_id();
    __builtin_amdgcn_wave_barrier();
    if (lane < CNT_N) { unsigned long long v = wc[lane]; if (v) atomicAdd(&global[lane], v); wc[lane] = 0ull; }
    __builtin_amdgcn_wave_barrier();
}
DEVINL void set_status(int32_t *status, int code)
{
    if (lane_id() == 0) atomicCAS(status, 0, code);
}
// make this wave's own global-memory writes visible to its later reads from other lanes
DEVINL void wave_sync_mem()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
