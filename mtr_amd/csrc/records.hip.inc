// records.hip.inc — where the records of a finished batch are, and the kernels that only serialise them.
//
// RecordView: read rd has its records in its max_rec slots, unless reads of the batch were run again with more room (resolve_overflow
// in mtr_abi.hip).  Then a per-read pointer table says where every read's records are, and only without that table is a count larger
// than the slots clamped to them.  Every kernel that reads a finished batch takes the view by value (record_view() makes it) and asks
// it for a read; the host sizes by the same rule (usable).
//   mtr_k_compact      one block per read: its records, 16 bytes a lane, to the read's offset in one dense array (mtr_fetch_results);
//   mtr_k_wire_sizes   a lane per read: the bytes of its records in the wire form;
//   mtr_k_wire_pack    one wavefront per read: its records in the wire form at the read's byte offset.
// Every result is written with ordinary vector stores.

struct ReadRecords { const DevRecord *rec; int n; };           // the records of one read and how many of them can be read
struct RecordView {
    const DevRecord *slots;                                    // max_rec slots per read
    const DevRecord *const *src_of;                            // per read: where its records are, or null = all in their own slots
    const int32_t *cnt;                                        // records FOUND per read
    int max_rec, n_reads;
    __host__ __device__ __forceinline__ int usable(int found) const { return !src_of && found > max_rec ? max_rec : found; }
    __device__ __forceinline__ ReadRecords read(int rd) const { return { src_of ? src_of[rd] : slots + (size_t)rd * (size_t)max_rec, usable(cnt[rd]) }; }
};

__global__ void mtr_k_compact(RecordView v, const int64_t *off, DevRecord *out)
{
    const int rd = blockIdx.x;
    if (rd >= v.n_reads) return;
    const auto [rec, c] = v.read(rd);
    const uint4 *src = (const uint4 *)rec;
    uint4 *dst = (uint4 *)(out + off[rd]);
    const size_t words = (size_t)c * sizeof(DevRecord) / 16;
    for (size_t t = threadIdx.x; t < words; t += blockDim.x) dst[t] = src[t];
}

// ---- wire form (include/mtr_hip.h): 14 int32 | rep_period unit bytes padded to 4 | rep_period int32 scores ---------
__device__ __forceinline__ int wire_period(const DevRecord *r) { int p = r->f[3]; return p < 0 ? 0 : (p > MTRC_MAX_PERIOD ? MTRC_MAX_PERIOD : p); }
__global__ void mtr_k_wire_sizes(RecordView v, int64_t *bytes)
{
    const int rd = blockIdx.x * blockDim.x + threadIdx.x;
    if (rd >= v.n_reads) return;
    const auto [src, c] = v.read(rd);
    int64_t b = 0;
    for (int t = 0; t < c; t++) { const int p = wire_period(src + t); b += 56 + ((p + 3) & ~3) + 4 * p; }
    bytes[rd] = b;
}
__global__ void mtr_k_wire_pack(RecordView v, const int64_t *off, uint8_t *out)
{
    // one wavefront per read; every piece of a wire record is a whole number of dwords at a dword-aligned offset
    const int rd = blockIdx.x;
    if (rd >= v.n_reads) return;
    const auto [src, c] = v.read(rd);
    uint32_t *dst = (uint32_t *)(out + off[rd]);
    for (int t = 0; t < c; t++) {
        const DevRecord *r = src + t;
        const int p = wire_period(r), uw = (p + 3) >> 2;
        const uint32_t *h = (const uint32_t *)r->f, *u = (const uint32_t *)r->unit, *sc = (const uint32_t *)r->unit_score;
        for (int q = threadIdx.x; q < 14 + uw + p; q += blockDim.x) {
            uint32_t w;
            if (q < 14) w = h[q];
            else if (q < 14 + uw) {
                w = u[q - 14];
                const int keep = p - 4 * (q - 14);                       // bytes of this word that belong to the unit
                if (keep < 4) w &= (1u << (8 * keep)) - 1u;
            } else w = sc[q - 14 - uw];
            dst[q] = w;
        }
        dst += 14 + uw + p;
    }
}
