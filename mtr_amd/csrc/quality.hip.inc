// quality.hip.inc — the Phred qualities of the resident batch (mtr_keep_qualities, mtr_attach_qualities_device) and their oriented windows
// (mtr_extract_window_qualities_device).  The batch's qualities are one byte per base in a buffer of the context: read r's at the exclusive sum
// of the lengths before it, values 0 .. MTR_QUAL_MAX.
//   mtr_k_qual_gather<ASCII>  one wavefront per read, 64 bytes a turn: the read's bytes at its own place in the source - the FASTQ file's quality
//                             line (ASCII: Phred + 33) or the caller's values - become its stored values
//   mtr_k_win_qual            one wavefront per row, 64 bytes a turn: mtr_k_win_gather's companion, the window's values reversed for orientation 1
// A lane reads its byte out of the aligned dword that holds it - the dword holds a byte of the source, so it lies in the dwords of the source's
// allocation, and the lanes of one dword share one request - and writes it with an ordinary byte store.
#pragma once
#include "device_util.hip.inc"

#define QL_MAX 93                  // MTR_QUAL_MAX
#define QL_MAX_GRID (1 << 16)

DEVINL uint32_t ql_byte_at(const uint8_t *p)
{
    const uint32_t r = (uint32_t)((uintptr_t)p & 3u);
    return (*(const uint32_t *)(p - r) >> (8u * r)) & 0xffu;
}

// src_line: per line of a FASTQ file its first byte (read r's quality line is line 4r + 3), or NULL: then src_off [n_reads] gives the reads' places
template <bool ASCII>
__global__ __launch_bounds__(64) void mtr_k_qual_gather(const uint8_t *src, const uint32_t *src_line, const int64_t *src_off, const int32_t *lens, const int64_t *qual_off,
                                                        int32_t n_reads, uint8_t *qual)
{
    const int lane = lane_id();
    for (int32_t r = (int32_t)blockIdx.x; r < n_reads; r += (int32_t)gridDim.x) {
        const uint8_t *in = src + (src_line ? (int64_t)src_line[4 * (int64_t)r + 3] : src_off[r]);
        uint8_t *out = qual + qual_off[r];
        const int32_t n = lens[r];
        for (int32_t t = lane; t < n; t += 64) {
            const int32_t v = (int32_t)ql_byte_at(in + t) - (ASCII ? 33 : 0);
            out[t] = (uint8_t)(v < 0 ? 0 : v > QL_MAX ? QL_MAX : v);
        }
    }
}

__global__ __launch_bounds__(64) void mtr_k_win_qual(const int32_t *row_read, const uint8_t *orientation, const int32_t *window, int64_t R, const uint8_t *qual,
                                                     const int64_t *qual_off, const int64_t *win_off, uint8_t *dst)
{
    const int lane = lane_id();
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        const uint8_t *q = qual + qual_off[row_read[r]];
        const int32_t lo = window[2 * r], hi = window[2 * r + 1];
        const bool rc = orientation[r] == 1;
        uint8_t *out = dst + win_off[r];
        for (int32_t t = lane; t < hi - lo; t += 64) out[t] = (uint8_t)ql_byte_at(q + (rc ? hi - 1 - t : lo + t));
    }
}
