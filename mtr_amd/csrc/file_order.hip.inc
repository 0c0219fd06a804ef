// file_order.hip.inc — file-order mode for reads that are already in device memory (mtr_upload_batch_device_in_file,
// mtr_upload_fasta_device_in_file): what a read finds beyond its own part of the reference's two whole-file buffers, made
// on the device from the packed words of the reads that left it there.  No base crosses to the host.
//
// The host keeps the staircase over lengths only and plans a batch with the same walk over it as the host feed (mtr_file_state::walk,
// plan_device, file_state.h); fo_launch (mtr_abi.hip) hands the kernels
//   segments   the stale tails of the batch, cut where their owner changes: FoSeg = (owner's words, owner's geometry, first
//              entry, first position), in entry order.  An owner is an earlier read of this batch (its words in the batch's
//              packed image) or a stair of the state (its words in the state's storage).
//   FoAfter    per read the owners' words of positions L and L + 1 of orgInputString (NULL: nobody wrote there, 'A' = 0).
//
// mtr_k_file_tail: one thread makes one tail entry, flattened over all entries of the batch.  A binary search over the segments'
// first entries finds the entry's segment, as pack.hip.inc finds a word's read; the thread then evaluates left_at() as
// mtr_file_state does on the host, from the owner's words and the MT19937 base stream.  Neighbouring lanes write neighbouring
// entries and read the same or neighbouring words / stream bytes.
// mtr_k_file_after: one thread per read (positions L and L + 1 may share a word, so one thread owns both).
// No LDS, no scratch.

#define MTR_FO_BLOCK 256

struct FoSeg {
    const uint32_t *words;      // the owner's 2-bit image (include/mtr_hip.h)
    int64_t t0;                 // the segment's first entry in the batch's tail
    int32_t p0;                 // that entry's position in inputString_w_rand
    int32_t L, r, N;            // the owner's geometry (n = L + 2r)
};
struct FoAfter { const uint32_t *w[2]; };

DEVINL int fo_base(const uint32_t *words, int p) { return (int)((words[p >> 4] >> (30 - 2 * (p & 15))) & 3u); }

DEVINL int fo_raw(const FoSeg &s, const uint8_t *__restrict__ mt, int n, int q)
{   // mtr_file_state::raw: the owner's buffer before the rolling encode
    if (q < s.r) return mt[s.N + q];
    if (q < s.r + s.L) return fo_base(s.words, q - s.r);
    if (q < n) return mt[s.N + q - s.L];
    return mt[q];                                                 // q < N
}

__global__ __launch_bounds__(MTR_FO_BLOCK) void mtr_k_file_tail(const FoSeg *__restrict__ segs, int32_t n_segs, int64_t entries,
                                                                const uint8_t *__restrict__ mt, uint16_t *__restrict__ tail)
{
    for (int64_t t = (int64_t)blockIdx.x * MTR_FO_BLOCK + threadIdx.x; t < entries; t += (int64_t)gridDim.x * MTR_FO_BLOCK) {
        int32_t lo = 0, hi = n_segs - 1;                          // the last segment whose first entry is <= t (t0 ascends)
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (segs[mid].t0 <= t) lo = mid; else hi = mid - 1;
        }
        const FoSeg s = segs[lo];
        const int n = s.L + 2 * s.r;
        const int p = s.p0 + (int)(t - s.t0);
        int v;
        if (p < n - 4) {                                          // mtr_file_state::left_at: the 5-mer code where one was formed
            v = 0;
#pragma unroll
            for (int k = 0; k < 5; k++) v = 4 * v + fo_raw(s, mt, n, p + k);
        } else v = fo_raw(s, mt, n, p);
        tail[t] = (uint16_t)v;
    }
}

// A read's own words past its last base are zero, so OR-ing is storing.  An owner of this batch may get its own two bases from
// another thread meanwhile: those land at ITS positions L, L + 1, never at the positions below its length that are read here.
__global__ __launch_bounds__(MTR_FO_BLOCK) void mtr_k_file_after(const FoAfter *__restrict__ own, const int64_t *__restrict__ woff,
                                                                 const int32_t *__restrict__ lens, int32_t n, uint32_t *packed,
                                                                 uint8_t *__restrict__ after)
{
    const int32_t i = (int32_t)(blockIdx.x * MTR_FO_BLOCK + threadIdx.x);
    if (i >= n) return;
    const FoAfter o = own[i];
    const int32_t L = lens[i];
    const uint32_t b0 = o.w[0] ? (uint32_t)fo_base(o.w[0], L) : 0u;
    const uint32_t b1 = o.w[1] ? (uint32_t)fo_base(o.w[1], L + 1) : 0u;
    uint32_t *w = packed + woff[i];
    const int32_t i0 = L >> 4, i1 = (L + 1) >> 4;
    const uint32_t v0 = b0 << (30 - 2 * (L & 15)), v1 = b1 << (30 - 2 * ((L + 1) & 15));
    if (i0 == i1) { if (v0 | v1) w[i0] |= v0 | v1; }
    else { if (v0) w[i0] |= v0; if (v1) w[i1] |= v1; }
    after[2 * (size_t)i] = (uint8_t)b0; after[2 * (size_t)i + 1] = (uint8_t)b1;
}
