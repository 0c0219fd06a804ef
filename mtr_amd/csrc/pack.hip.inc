// pack.hip.inc — mtr_upload_batch_device: reads that are already in device memory, one byte per base, packed on the device
// into the 2-bit image of include/mtr_hip.h ("the host's own packing"), bit for bit what mtr_pack_read writes.
//
// One thread makes one 32-bit word (16 bases), flattened over all words of the batch: a binary search over the word offsets
// finds the word's read, so neighbouring lanes read neighbouring 16-byte spans of the text and write neighbouring words, and a
// batch of any length mix spreads evenly.  Words past the read's last base (the 3 zero words, and the tail of the last partial
// word) come out 0.  Every byte inside a read is checked; the first read (lowest index) holding a byte that is not a base of the
// chosen kind is atomicMin'ed into *bad (the host names it).  No LDS, no scratch.

#define MTR_PACK_BLOCK 256

// one text byte -> its code 0..3; ok is cleared when the byte is not a base of the chosen kind
template <bool ASCII>
__device__ __forceinline__ uint32_t mtr_pack_code(uint32_t c, bool &ok)
{
    if (ASCII) {
        const uint32_t u = c | 0x20u;                                 // exact membership in {A,C,G,T,a,c,g,t}: u folds only X and X^0x20
        ok = ok && (u == 'a' || u == 'c' || u == 'g' || u == 't');
        return ((c >> 1) ^ (c >> 2)) & 3u;                            // A/a -> 0, C/c -> 1, G/g -> 2, T/t -> 3
    }
    ok = ok && c <= 3u;
    return c & 3u;
}

// 4 text bytes (little-endian in y: byte 0 = the earlier base) appended to v as 4 codes (earlier base in higher bits)
template <bool ASCII>
__device__ __forceinline__ uint32_t mtr_pack_bytes4(uint32_t y, uint32_t v, bool &ok)
{
#pragma unroll
    for (int t = 0; t < 4; t++) v = (v << 2) | mtr_pack_code<ASCII>((y >> (8 * t)) & 0xffu, ok);
    return v;
}

template <bool ASCII>
__global__ __launch_bounds__(MTR_PACK_BLOCK) void mtr_k_pack_text(const uint8_t *__restrict__ text, const int64_t *__restrict__ toff,
                                                                  const int32_t *__restrict__ lens, const int64_t *__restrict__ woff,
                                                                  int32_t n, int64_t words, uint32_t *__restrict__ packed, int32_t *__restrict__ bad)
{
    for (int64_t w = (int64_t)blockIdx.x * MTR_PACK_BLOCK + threadIdx.x; w < words; w += (int64_t)gridDim.x * MTR_PACK_BLOCK) {
        int32_t lo = 0, hi = n - 1;                                   // the last read whose first word is <= w (woff ascends)
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (woff[mid] <= w) lo = mid; else hi = mid - 1;
        }
        const int32_t L = lens[lo];
        const int32_t p0 = (int32_t)(w - woff[lo]) << 4;              // first base of this word (< L + 64 <= MTR_MAX_READ_LENGTH + 64)
        const int32_t nb = min(max(L - p0, 0), 16);
        const uint8_t *s = text + toff[lo] + p0;
        uint32_t v = 0;
        bool ok = true;
        if (nb == 16) {
            // 16 bases through aligned dword loads: each dword holds at least one byte of the read, so none leaves the text's
            // allocation; the bytes of a dword outside the read are shifted out unseen.
            const uint32_t r = (uint32_t)((uintptr_t)s & 3u);
            const uint32_t *d = (const uint32_t *)(s - r);
            uint32_t x0 = d[0], x1 = d[1], x2 = d[2], x3 = d[3];
            if (r) {
                const uint32_t x4 = d[4];
                x0 = __builtin_amdgcn_alignbyte(x1, x0, r); x1 = __builtin_amdgcn_alignbyte(x2, x1, r);
                x2 = __builtin_amdgcn_alignbyte(x3, x2, r); x3 = __builtin_amdgcn_alignbyte(x4, x3, r);
            }
            v = mtr_pack_bytes4<ASCII>(x0, v, ok); v = mtr_pack_bytes4<ASCII>(x1, v, ok);
            v = mtr_pack_bytes4<ASCII>(x2, v, ok); v = mtr_pack_bytes4<ASCII>(x3, v, ok);
        } else {
            for (int32_t t = 0; t < nb; t++) {                        // the read's last, partial word (nb = 0: a zero word behind the read)
                v |= mtr_pack_code<ASCII>(s[t], ok) << (30 - 2 * t);
            }
        }
        if (!ok) atomicMin(bad, lo);
        packed[w] = v;
    }
}
