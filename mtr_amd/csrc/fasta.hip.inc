// fasta.hip.inc — mtr_parse_fasta_device / mtr_upload_fasta_device: a FASTA file's bytes in device memory become the reads, their
// lengths and their IDs on the device, by the rules of the reference's reader (handle_one_file.c:169-269, restated in the head comment
// of mtr_amd/host/fasta.c).  For byte i of n:
//   line start    ls(i) = the index of the last LF before i, plus 1 (0 if there is none);
//   fgets window  the reference reads with fgets(s, 4096): windows start at ls + k * 4095, ws(i) = i - (i - ls(i)) % 4095; a window whose
//                 first byte is '>' is a HEADER window, every other one a SEQUENCE window;
//   dead          NUL, LF and CR are terminators; a byte is dead if a terminator lies in [ws(i), i];
//   base          a byte of a sequence window that is not dead is a candidate: one of ACGTacgt is a BASE, any other a BAD character;
//   ID            of a header window: the bytes behind '>' up to the first terminator of the window (at most 4094);
//   record        a base belongs to record max(h - 1, 0), h = the header windows that start at or before it;
//   stop          the first in file order of: a bad character; a header that closes a record without bases (EMPTY); the 1 000 000th base
//                 of a record (TOOLONG).  The reads are the records closed - by the next header window or the end of the file - before it.
// All of it is prefix scans over the bytes, organised as tile-local scan, scan of the tile sums, apply.  A tile is MTR_FASTA_TILE_BYTES of
// the file, one workgroup of 256 threads, 16 bytes a thread.  No workgroup waits for another: order is kernel boundaries on the stream.
//   mtr_k_fasta_lines        per tile the last LF and the last terminator (positions + 1, 0 = none);
//   mtr_k_fasta_scan_lines   ONE workgroup: their exclusive running maxima over the tiles = every tile's line start and last terminator;
//   mtr_k_fasta_tile<0>      with those every byte knows its window, so whether it is a base or starts a header: per tile the bases, the
//                            headers, and the bases in front of its last header;
//   mtr_k_fasta_scan_counts  ONE workgroup: per tile the bases and headers before it, and the base count at which the record that is open
//                            at its first byte began (a running maximum: base counts only grow); the totals;
//   mtr_k_fasta_tile<1>      the same walk with global counts: per header its position, the bases before it, its ID's length; the stop events,
//                            atomicMin'ed as position * 4 + kind into one 64-bit word;
//   mtr_k_scan_offsets       (report_align.hip.inc) the IDs' offsets;
//   mtr_k_fasta_finish       one thread: the reads before the stop (a binary search over the header positions) and the sizes; for a
//                            window of a longer input (more, below) the records that a header window closed;
//   mtr_k_fasta_reads / mtr_k_fasta_ids / mtr_k_fasta_tile<2>   the reads' offsets and lengths, their IDs gathered, the bases compacted (through
//                            LDS, so that a tile's bases leave as one run of neighbouring bytes) - the file's own bytes, which
//                            mtr_k_pack_text takes as MTR_TEXT_ASCII.
// The file is read with aligned dword loads as mtr_k_pack_text reads its text: every dword loaded holds at least one byte of the file; the
// bytes past the end of the last 16-byte span are loaded one by one.  Positions and counts are 32-bit: the entry points refuse more than
// INT32_MAX bytes.  Every result is written with ordinary vector stores.
// A WINDOW of a longer input (mtr_parse_fasta_device_window, more = 1): the buffer is the input's first n bytes and what follows is
// unknown.  All of the above is a function of the bytes before a position, so a stop found in the window is a stop of the input and is
// reported as ever.  Without one only the end of the file is missing: the last record stays open and is not a read, end =
// MTR_FASTA_END_MORE, end_pos = where its header window starts (0 for the window's first record, which owns the bases in front of its
// header as well).  A header window starts an fgets window, so a parse that begins there puts every later window where this one would.
// Only mtr_k_fasta_finish knows the mode.

#define MTR_FASTA_TILE_BYTES 4096
#define MTR_FASTA_BLOCK 256                                    // x 16 bytes a thread = one tile
#define MTR_FASTA_WINDOW 4095                                  // what fgets(s, 4096) reads at most
#define MTR_FASTA_SCAN_BLOCK 1024
#define MTR_FASTA_NO_EVENT 0xffffffffffffffffull

struct FastaArgs {
    const uint8_t *fa; int32_t n, n_tiles;
    uint32_t *t_nl, *t_term;                                   // [n_tiles] last LF / terminator of the tile; after the scan: before the tile (position + 1)
    uint32_t *t_cnt, *t_last;                                  // [n_tiles] bases | headers << 16; bases in front of the tile's last header + 1 (0 = no header)
    uint32_t *t_base, *t_hdr, *t_rs;                           // [n_tiles] bases / headers before the tile; the base count at which the open record began
    uint32_t *totals;                                          // [2] bases, headers of the file
    int32_t *h_pos, *h_idlen; uint32_t *h_base; uint32_t n_heads;      // per header window: where it starts, its ID's length, the bases before it
    unsigned long long *event;                                 // the first stop: position * 4 + MTR_FASTA_END_*
    uint8_t *text; uint32_t n_bases;                           // mtr_k_fasta_tile<2>: the bases of the reads before the stop
};

__device__ __forceinline__ uint32_t fa_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Inclusive scan (sum, or maximum with 0 as "none") over the NW wavefronts of the workgroup; excl = the scan without the thread's own
// value, total = the workgroup's.  Every thread of the workgroup calls it; s: NW words of LDS, free again on return.
template <bool MAX, int NW>
__device__ __forceinline__ uint32_t fa_block_scan(uint32_t v, uint32_t *s, uint32_t &excl, uint32_t &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= d) incl = MAX ? fa_max(incl, o) : incl + o; }
    uint32_t prev = __shfl_up(incl, 1, 64);
    if (lane == 0) prev = 0;
    if (lane == 63) s[w] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (int k = 0; k < NW; k++) {
        const uint32_t x = s[k];
        if (k < w) before = MAX ? fa_max(before, x) : before + x;
        total = MAX ? fa_max(total, x) : total + x;
    }
    __syncthreads();
    excl = MAX ? fa_max(before, prev) : before + prev;
    return MAX ? fa_max(before, incl) : before + incl;
}

// the thread's 16 bytes of the file from byte i0 on, little-endian in x; returns how many of them exist (0 .. 16)
__device__ __forceinline__ int fa_load16(const uint8_t *fa, int32_t n, int64_t i0, uint32_t (&x)[4])
{
    x[0] = x[1] = x[2] = x[3] = 0u;
    if (i0 >= (int64_t)n) return 0;
    const uint8_t *s = fa + i0;
    if (i0 + 16 <= (int64_t)n) {
        // aligned dword loads: each dword holds at least one of the 16 bytes, so none leaves the dwords of the file
        const uint32_t r = (uint32_t)((uintptr_t)s & 3u);
        const uint32_t *d = (const uint32_t *)(s - r);
        x[0] = d[0]; x[1] = d[1]; x[2] = d[2]; x[3] = d[3];
        if (r) {
            const uint32_t x4 = d[4];
            x[0] = __builtin_amdgcn_alignbyte(x[1], x[0], r); x[1] = __builtin_amdgcn_alignbyte(x[2], x[1], r);
            x[2] = __builtin_amdgcn_alignbyte(x[3], x[2], r); x[3] = __builtin_amdgcn_alignbyte(x4, x[3], r);
        }
        return 16;
    }
    const int nv = (int)((int64_t)n - i0);                      // the file's last, partial span
#pragma unroll
    for (int j = 0; j < 16; j++) if (j < nv) x[j >> 2] |= (uint32_t)s[j] << (8 * (j & 3));
    return nv;
}

__device__ __forceinline__ bool fa_is_term(uint32_t c) { return c == 0u || c == 10u || c == 13u; }

// the last LF and the last terminator among the thread's bytes, as position + 1 (0 = none)
__device__ __forceinline__ void fa_line_marks(const uint32_t (&x)[4], int nv, int64_t i0, uint32_t &nl, uint32_t &tm)
{
    nl = 0u; tm = 0u;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t c = (x[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (j < nv) {
            const uint32_t p1 = (uint32_t)(i0 + j) + 1u;
            if (c == 10u) nl = p1;
            if (fa_is_term(c)) tm = p1;
        }
    }
}

__global__ __launch_bounds__(MTR_FASTA_BLOCK) void mtr_k_fasta_lines(FastaArgs a)
{
    __shared__ uint32_t s[4];
    const int tile = blockIdx.x;
    const int64_t i0 = (int64_t)tile * MTR_FASTA_TILE_BYTES + (int64_t)threadIdx.x * 16;
    uint32_t x[4], nl, tm, ex, tot_nl, tot_tm;
    const int nv = fa_load16(a.fa, a.n, i0, x);
    fa_line_marks(x, nv, i0, nl, tm);
    fa_block_scan<true, 4>(nl, s, ex, tot_nl);
    fa_block_scan<true, 4>(tm, s, ex, tot_tm);
    if (threadIdx.x == 0) { a.t_nl[tile] = tot_nl; a.t_term[tile] = tot_tm; }
}

// in place: t_nl[t] / t_term[t] = the maximum over the tiles before t
__global__ __launch_bounds__(MTR_FASTA_SCAN_BLOCK) void mtr_k_fasta_scan_lines(FastaArgs a)
{
    __shared__ uint32_t s[16];
    uint32_t c_nl = 0u, c_tm = 0u;
    for (int32_t c = 0; c < a.n_tiles; c += MTR_FASTA_SCAN_BLOCK) {
        const int32_t t = c + (int32_t)threadIdx.x;
        const bool in = t < a.n_tiles;
        uint32_t ex_nl, ex_tm, tot_nl, tot_tm;
        fa_block_scan<true, 16>(in ? a.t_nl[t] : 0u, s, ex_nl, tot_nl);
        fa_block_scan<true, 16>(in ? a.t_term[t] : 0u, s, ex_tm, tot_tm);
        if (in) { a.t_nl[t] = fa_max(c_nl, ex_nl); a.t_term[t] = fa_max(c_tm, ex_tm); }
        c_nl = fa_max(c_nl, tot_nl); c_tm = fa_max(c_tm, tot_tm);
    }
}

// The reader's state in front of a byte: its place in the fgets window, whether that window is a header window, whether a terminator
// of the window lies before it.
struct FaState { int32_t w; bool hdrwin, dead; };
// What a byte is: the first byte of a header window; a base; a bad character; the byte that ends its header window's ID (idlen >= 0).
struct FaByte { bool hdr_start, base, bad; int32_t idlen; };

__device__ __forceinline__ FaByte fa_step(FaState &s, uint32_t c, bool last_of_file)
{
    FaByte b;
    b.hdr_start = s.w == 0 && c == (uint32_t)'>';
    if (s.w == 0) { s.hdrwin = b.hdr_start; s.dead = false; }
    const bool term = fa_is_term(c), first_term = term && !s.dead;
    s.dead = s.dead || term;
    const uint32_t u = c | 0x20u;                                 // exact membership in {A,C,G,T,a,c,g,t} (mtr_pack_code)
    const bool cand = !s.hdrwin && !s.dead, acgt = u == 'a' || u == 'c' || u == 'g' || u == 't';
    b.base = cand && acgt;
    b.bad = cand && !acgt;
    b.idlen = -1;
    if (s.hdrwin) {
        if (first_term) b.idlen = s.w - 1;                        // the bytes between '>' and the terminator
        else if (!s.dead && (s.w == MTR_FASTA_WINDOW - 1 || last_of_file)) b.idlen = s.w;      // the window ends without one
    }
    s.w = (c == 10u || s.w == MTR_FASTA_WINDOW - 1) ? 0 : s.w + 1;
    return b;
}

// MODE 0: the tile's counts.  MODE 1: the headers' columns and the stop events.  MODE 2: the bases, compacted.
template <int MODE>
__global__ __launch_bounds__(MTR_FASTA_BLOCK) void mtr_k_fasta_tile(FastaArgs a)
{
    __shared__ uint32_t s[4];
    __shared__ uint8_t s_text[MODE == 2 ? MTR_FASTA_TILE_BYTES : 4];
    const int tile = blockIdx.x;
    const int64_t i0 = (int64_t)tile * MTR_FASTA_TILE_BYTES + (int64_t)threadIdx.x * 16;
    uint32_t x[4], nl, tm, nl_ex, tm_ex, tot;
    const int nv = fa_load16(a.fa, a.n, i0, x);
    fa_line_marks(x, nv, i0, nl, tm);
    fa_block_scan<true, 4>(nl, s, nl_ex, tot);
    fa_block_scan<true, 4>(tm, s, tm_ex, tot);
    nl_ex = fa_max(nl_ex, a.t_nl[tile]);                          // = the start of the line the thread's first byte is on
    tm_ex = fa_max(tm_ex, a.t_term[tile]);
    FaState st0 = { 0, false, false };
    if (nv > 0) {
        const int32_t p0 = (int32_t)i0;
        st0.w = (p0 - (int32_t)nl_ex) % MTR_FASTA_WINDOW;
        const int32_t ws = p0 - st0.w;
        st0.hdrwin = st0.w != 0 && a.fa[ws] == (uint8_t)'>';      // (a window that starts in the thread's own bytes is met on the walk)
        st0.dead = tm_ex > (uint32_t)ws;
    }
    // first walk: the thread's bases, headers, and the bases in front of its last header
    uint32_t nb = 0u, nh = 0u, lastb = 0u;
    {
        FaState st = st0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (j < nv) {
                const FaByte b = fa_step(st, (x[j >> 2] >> (8 * (j & 3))) & 0xffu, false);
                if (b.hdr_start) { nh++; lastb = nb + 1u; }
                if (b.base) nb++;
            }
        }
    }
    uint32_t ex, cnt;
    fa_block_scan<false, 4>(nb | (nh << 16), s, ex, cnt);
    const uint32_t exb = ex & 0xffffu, exh = ex >> 16;
    if (MODE == 0) {
        uint32_t last;
        fa_block_scan<true, 4>(lastb ? exb + lastb : 0u, s, ex, last);
        if (threadIdx.x == 0) { a.t_cnt[tile] = cnt; a.t_last[tile] = last; }
    }
    if (MODE == 1) {
        uint32_t B = a.t_base[tile] + exb, h = a.t_hdr[tile] + exh, rs, rs_tot;
        // where the record that is open behind the thread's last header began (the first header of the file opens none: 0)
        fa_block_scan<true, 4>(nh && h + nh > 1u ? B + lastb - 1u : 0u, s, rs, rs_tot);
        rs = fa_max(rs, a.t_rs[tile]);
        unsigned long long ev = MTR_FASTA_NO_EVENT;
        FaState st = st0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (j < nv) {
                const int32_t i = (int32_t)i0 + j;
                const FaByte b = fa_step(st, (x[j >> 2] >> (8 * (j & 3))) & 0xffu, i == a.n - 1);
                unsigned long long e = MTR_FASTA_NO_EVENT;
                if (b.hdr_start) {
                    if (h < a.n_heads) { a.h_pos[h] = i; a.h_base[h] = B; }
                    if (h >= 1u) { if (B == rs) e = ((unsigned long long)i << 2) | MTR_FASTA_END_EMPTY; rs = B; }
                    h++;
                }
                if (b.base) { if (B - rs == (uint32_t)(MTR_MAX_INPUT_LENGTH - 1)) e = ((unsigned long long)i << 2) | MTR_FASTA_END_TOOLONG; B++; }
                if (b.bad) e = ((unsigned long long)i << 2) | MTR_FASTA_END_BADCHAR;
                if (b.idlen >= 0 && h - 1u < a.n_heads) a.h_idlen[h - 1u] = b.idlen;
                ev = e < ev ? e : ev;
            }
        }
        for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(ev, d, 64); ev = o < ev ? o : ev; }
        if ((threadIdx.x & 63) == 0 && ev != MTR_FASTA_NO_EVENT) atomicMin(a.event, ev);
    }
    if (MODE == 2) {
        const uint32_t B0 = a.t_base[tile];
        uint32_t q = exb;
        FaState st = st0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (j < nv) {
                const uint32_t c = (x[j >> 2] >> (8 * (j & 3))) & 0xffu;
                const FaByte b = fa_step(st, c, false);
                if (b.base && q < MTR_FASTA_TILE_BYTES) s_text[q++] = (uint8_t)c;
            }
        }
        __syncthreads();
        const uint32_t nbt = cnt & 0xffffu, keep = B0 >= a.n_bases ? 0u : (a.n_bases - B0 < nbt ? a.n_bases - B0 : nbt);
        for (uint32_t k = threadIdx.x; k < keep; k += MTR_FASTA_BLOCK) a.text[(size_t)B0 + k] = s_text[k];
    }
}

// per tile the bases and headers before it and where the record open at its first byte began; totals[0 .. 1] = the file's bases, headers
__global__ __launch_bounds__(MTR_FASTA_SCAN_BLOCK) void mtr_k_fasta_scan_counts(FastaArgs a)
{
    __shared__ uint32_t s[16];
    uint32_t c_b = 0u, c_h = 0u, c_rs = 0u;
    for (int32_t c = 0; c < a.n_tiles; c += MTR_FASTA_SCAN_BLOCK) {
        const int32_t t = c + (int32_t)threadIdx.x;
        const bool in = t < a.n_tiles;
        const uint32_t cnt = in ? a.t_cnt[t] : 0u, last = in ? a.t_last[t] : 0u, nb = cnt & 0xffffu, nh = cnt >> 16;
        uint32_t exb, exh, exv, totb, toth, totv;
        fa_block_scan<false, 16>(nb, s, exb, totb);
        fa_block_scan<false, 16>(nh, s, exh, toth);
        const uint32_t P = c_b + exb, H = c_h + exh;
        fa_block_scan<true, 16>(last && H + nh > 1u ? P + last - 1u : 0u, s, exv, totv);
        if (in) { a.t_base[t] = P; a.t_hdr[t] = H; a.t_rs[t] = fa_max(c_rs, exv); }
        c_b += totb; c_h += toth; c_rs = fa_max(c_rs, totv);
    }
    if (threadIdx.x == 0) { a.totals[0] = c_b; a.totals[1] = c_h; }
}

// The reads before the stop and the sizes.  n_heads = the header windows, or 1 for a file without one: its only record has the ID ""
// (the host zeroes that header's columns).  Record r has the ID of header r, begins at base h_base[r] (record 0 at base 0: the bases
// in front of the first header join it) and is closed by header r + 1 or by the end of the file.
// more: the input goes on behind the buffer - without a stop the last record is open: not a read, and the next window starts on its header.
__global__ __launch_bounds__(64) void mtr_k_fasta_finish(FastaArgs a, int32_t n_heads, int32_t more, const int64_t *id_off, mtr_fasta_info *info)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long ev = *a.event;
    const uint32_t total = a.totals[0];
    int32_t n_reads, end, bad = 0; int64_t end_pos;
    if (ev == MTR_FASTA_NO_EVENT && more) {
        n_reads = n_heads - 1;
        end = MTR_FASTA_END_MORE;
        end_pos = n_reads > 0 ? (int64_t)a.h_pos[n_reads] : 0;
    } else if (ev == MTR_FASTA_NO_EVENT) {
        const uint32_t last = total - (n_heads > 1 ? a.h_base[n_heads - 1] : 0u);
        n_reads = n_heads - 1 + (last > 0u ? 1 : 0);
        end = last > 0u ? MTR_FASTA_END_EOF : MTR_FASTA_END_EMPTY;
        end_pos = a.n;
    } else {
        end = (int32_t)(ev & 3ull); end_pos = (int64_t)(ev >> 2);
        if (end == MTR_FASTA_END_BADCHAR) bad = a.fa[end_pos];
        int32_t lo = 1, hi = n_heads;                             // the first header from 1 on that does not start before the stop
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if ((int64_t)a.h_pos[mid] < end_pos) lo = mid + 1; else hi = mid; }
        n_reads = lo - 1;
    }
    info->n_reads = n_reads; info->end = end; info->bad_char = bad; info->reserved = 0;
    info->end_pos = end_pos;
    info->n_bases = n_reads == 0 ? 0 : (n_reads < n_heads ? (int64_t)a.h_base[n_reads] : (int64_t)total);
    info->id_bytes = id_off[n_reads];
}

__global__ __launch_bounds__(256) void mtr_k_fasta_reads(FastaArgs a, int32_t n_heads, int32_t n_reads, int64_t *offsets, int32_t *lens)
{
    for (int32_t r = (int32_t)(blockIdx.x * 256u + threadIdx.x); r < n_reads; r += (int32_t)(gridDim.x * 256u)) {
        const uint32_t b0 = r ? a.h_base[r] : 0u, b1 = r + 1 < n_heads ? a.h_base[r + 1] : a.totals[0];
        offsets[r] = (int64_t)b0; lens[r] = (int32_t)(b1 - b0);
    }
}

// one wavefront per read: its ID's bytes from behind the header's '>' to ids[id_off[r] ..]
__global__ __launch_bounds__(64) void mtr_k_fasta_ids(FastaArgs a, int32_t n_reads, const int64_t *id_off, uint8_t *ids)
{
    for (int32_t r = (int32_t)blockIdx.x; r < n_reads; r += (int32_t)gridDim.x) {
        const int64_t o = id_off[r], len = id_off[r + 1] - o;
        const uint8_t *src = a.fa + a.h_pos[r] + 1;
        for (int64_t k = threadIdx.x; k < len; k += 64) ids[o + k] = src[k];
    }
}
