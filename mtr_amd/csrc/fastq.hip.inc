// fastq.hip.inc — mtr_parse_fastq_device / mtr_upload_fastq_device: a FASTQ file's bytes in device memory become the reads, their lengths
// and their IDs on the device.  The reference has no FASTQ reader; the rules are this project's: strict four-line FASTQ, as the
// basecallers write it.
//   lines         line 0 starts at byte 0; line l + 1 starts behind the l-th LF, if a byte exists there (no fgets windows here);
//   content       a line's content is its bytes in front of its first NUL, LF or CR - the FASTA rules' terminators; a terminator hides the
//                 rest of its line;
//   record r      is lines 4r .. 4r + 3:
//                   header     content begins with '@'; the ID is the content behind it, spaces included, and may be empty;
//                   sequence   every content byte is one of ACGTacgt;
//                   separator  content begins with '+'; the rest is ignored;
//                   quality    content is as long as the sequence's content; its bytes are not looked at otherwise ('@', '>' and '+' are
//                              legal first quality characters and are not taken for a header);
//   stop          the input stops at the first of these in file order:
//                   MTR_FASTA_END_BADCHAR  a sequence content byte outside ACGTacgt ('N' included): end_pos at that byte, bad_char holds it;
//                   MTR_FASTA_END_TOOLONG  the 1 000 000th base of a sequence line: end_pos at that base;
//                   MTR_FASTA_END_EMPTY    a sequence line with empty content: end_pos = the line's first byte;
//                   MTR_FASTA_END_FORMAT   a header line not beginning with '@' or a separator line not beginning with '+': end_pos = the
//                                          line's first byte; a quality line whose content length differs from the sequence's: end_pos =
//                                          the line's first byte; the file ends inside a record (fewer than four of its lines begin):
//                                          end_pos = n_bytes.  A blank line behind the last record is a header line without '@';
//   reads         the records whose four lines are complete and correct before the stop; a last quality line without LF is complete;
//   end of file   no stop: MTR_FASTA_END_EOF.  (n_bytes == 0 never gets here: no reads, MTR_FASTA_END_EMPTY, as for FASTA.)
// Organised as fasta.hip.inc is, with its helpers (fa_load16, fa_line_marks, fa_block_scan): a tile is MTR_FASTA_TILE_BYTES of the file, one
// workgroup of 256 threads, 16 bytes a thread; no workgroup waits for another, order is kernel boundaries on the stream.
//   mtr_k_fastq_lines        per tile its LFs, its last LF and its last terminator (positions + 1, 0 = none);
//   mtr_k_fastq_scan_lines   ONE workgroup: per tile the lines before it, its line start and the last terminator before it; the file's lines;
//   mtr_k_fastq_tile<0>      with those every byte knows its line, hence line % 4: the line table - l_start[l] by the thread that owns the
//                            line's first byte, l_end[l] (the end of the content) by the thread that owns its first terminator, n for a
//                            last line without one - and the stops inside sequence lines, atomicMin'ed as position * 8 + kind into one
//                            64-bit word;
//   mtr_k_fastq_records      one thread a record: the four lines checked against the table (the other stops), the record's header
//                            position, ID length and sequence length;
//   mtr_k_scan_offsets       (report_align.hip.inc) the IDs' offsets and the bases' offsets, over all records;
//   mtr_k_fastq_finish       one thread: the reads before the stop (a binary search over the line starts) and the sizes;
//   mtr_k_fastq_reads / mtr_k_fasta_ids / mtr_k_fastq_tile<1>   the reads' offsets and lengths, their IDs gathered (fasta.hip.inc's kernel:
//                            a header is a position and an ID length there too), the bases compacted through LDS as mtr_k_fasta_tile<2>
//                            does.
// A sequence line is contiguous in the file, so mtr_upload_fastq_device compacts nothing: mtr_k_fastq_reads gives it the sequence lines'
// starts and mtr_k_pack_text packs the file's own bytes from there.
// A WINDOW of a longer input (mtr_parse_fastq_device_window, more = 1): the buffer is the input's first n bytes.  A stop that the bytes
// before it decide is a stop of the input and is reported as ever.  Two stops need more than that and are not raised: "the file ends
// inside a record", and the length of a quality line whose LF is not in the window.  Without a stop the reads are the records whose
// quality line's LF is in the window, end = MTR_FASTA_END_MORE, end_pos = the byte behind the last such LF.  mtr_k_fastq_records and
// mtr_k_fastq_finish know the mode.
// Loads are fa_load16's aligned dwords (the file's last partial span bytewise); positions and counts are 32-bit; every result is written
// with ordinary vector stores.

struct FastqArgs {
    const uint8_t *fq; int32_t n, n_tiles;
    uint32_t *t_cnt, *t_nl, *t_term;                           // [n_tiles] the tile's LFs, last LF, last terminator (position + 1); after the scan: before the tile
    uint32_t *totals;                                          // [1] the lines of the file
    uint32_t *l_start, *l_end; uint32_t n_lines;               // per line: its first byte, the end of its content
    int32_t *r_pos, *r_idlen, *r_len; uint32_t n_recs;         // per record: its header line's first byte, its ID's length, its sequence's length
    unsigned long long *event;                                 // the first stop: position * 8 + MTR_FASTA_END_*
    const int64_t *b_off;                                      // [n_recs + 1] the exclusive sum of r_len
    uint8_t *text; uint32_t n_reads;                           // mtr_k_fastq_tile<1>: the bases of the reads before the stop
};

// the LFs among the thread's bytes
__device__ __forceinline__ uint32_t fq_count_lf(const uint32_t (&x)[4], int nv)
{
    uint32_t cnt = 0u;
#pragma unroll
    for (int j = 0; j < 16; j++) if (j < nv && ((x[j >> 2] >> (8 * (j & 3))) & 0xffu) == 10u) cnt++;
    return cnt;
}

__device__ __forceinline__ unsigned long long fq_event(uint32_t pos, int kind) { return ((unsigned long long)pos << 3) | (unsigned long long)kind; }

// the workgroup's earliest stop into *event: one atomic a wavefront that has one
__device__ __forceinline__ void fq_post(unsigned long long ev, unsigned long long *event)
{
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(ev, d, 64); ev = o < ev ? o : ev; }
    if ((threadIdx.x & 63) == 0 && ev != MTR_FASTA_NO_EVENT) atomicMin(event, ev);
}

__global__ __launch_bounds__(MTR_FASTA_BLOCK) void mtr_k_fastq_lines(FastqArgs a)
{
    __shared__ uint32_t s[4];
    const int tile = blockIdx.x;
    const int64_t i0 = (int64_t)tile * MTR_FASTA_TILE_BYTES + (int64_t)threadIdx.x * 16;
    uint32_t x[4], nl, tm, ex, tot_nl, tot_tm, tot_cnt;
    const int nv = fa_load16(a.fq, a.n, i0, x);
    fa_line_marks(x, nv, i0, nl, tm);
    fa_block_scan<true, 4>(nl, s, ex, tot_nl);
    fa_block_scan<true, 4>(tm, s, ex, tot_tm);
    fa_block_scan<false, 4>(fq_count_lf(x, nv), s, ex, tot_cnt);
    if (threadIdx.x == 0) { a.t_cnt[tile] = tot_cnt; a.t_nl[tile] = tot_nl; a.t_term[tile] = tot_tm; }
}

// in place: t_cnt[t] = the LFs of the tiles before t, t_nl[t] / t_term[t] = the maximum over them; totals[0] = the lines of the file
__global__ __launch_bounds__(MTR_FASTA_SCAN_BLOCK) void mtr_k_fastq_scan_lines(FastqArgs a)
{
    __shared__ uint32_t s[16];
    uint32_t c_cnt = 0u, c_nl = 0u, c_tm = 0u;
    for (int32_t c = 0; c < a.n_tiles; c += MTR_FASTA_SCAN_BLOCK) {
        const int32_t t = c + (int32_t)threadIdx.x;
        const bool in = t < a.n_tiles;
        uint32_t ex_cnt, ex_nl, ex_tm, tot_cnt, tot_nl, tot_tm;
        fa_block_scan<false, 16>(in ? a.t_cnt[t] : 0u, s, ex_cnt, tot_cnt);
        fa_block_scan<true, 16>(in ? a.t_nl[t] : 0u, s, ex_nl, tot_nl);
        fa_block_scan<true, 16>(in ? a.t_term[t] : 0u, s, ex_tm, tot_tm);
        if (in) { a.t_cnt[t] = c_cnt + ex_cnt; a.t_nl[t] = fa_max(c_nl, ex_nl); a.t_term[t] = fa_max(c_tm, ex_tm); }
        c_cnt += tot_cnt; c_nl = fa_max(c_nl, tot_nl); c_tm = fa_max(c_tm, tot_tm);
    }
    // one line per LF, and one more behind the last LF (or from byte 0) if a byte exists there
    if (threadIdx.x == 0) a.totals[0] = c_cnt + (c_nl < (uint32_t)a.n ? 1u : 0u);
}

// The reader's state in front of a byte: its line, where that line starts, whether a terminator of the line lies before it.
struct FqState { uint32_t ln, ls; bool dead; };

// MODE 0: the line table and the stops inside sequence lines.  MODE 1: the bases of the reads before the stop, compacted.
template <int MODE>
__global__ __launch_bounds__(MTR_FASTA_BLOCK) void mtr_k_fastq_tile(FastqArgs a)
{
    __shared__ uint32_t s[4];
    __shared__ uint32_t s_first;
    __shared__ uint8_t s_text[MODE == 1 ? MTR_FASTA_TILE_BYTES : 4];
    const int tile = blockIdx.x;
    const int64_t i0 = (int64_t)tile * MTR_FASTA_TILE_BYTES + (int64_t)threadIdx.x * 16;
    uint32_t x[4], nl, tm, nl_ex, tm_ex, ln_ex, tot;
    const int nv = fa_load16(a.fq, a.n, i0, x);
    fa_line_marks(x, nv, i0, nl, tm);
    fa_block_scan<true, 4>(nl, s, nl_ex, tot);
    fa_block_scan<true, 4>(tm, s, tm_ex, tot);
    fa_block_scan<false, 4>(fq_count_lf(x, nv), s, ln_ex, tot);
    FqState st0;
    st0.ln = a.t_cnt[tile] + ln_ex;
    st0.ls = fa_max(nl_ex, a.t_nl[tile]);                         // = the start of the line the thread's first byte is on
    st0.dead = fa_max(tm_ex, a.t_term[tile]) > st0.ls;
    if (MODE == 0) {
        unsigned long long ev = MTR_FASTA_NO_EVENT;
        FqState st = st0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (j < nv) {
                const uint32_t c = (x[j >> 2] >> (8 * (j & 3))) & 0xffu, i = (uint32_t)i0 + (uint32_t)j;
                const bool listed = st.ln < a.n_lines, term = fa_is_term(c);
                if (i == st.ls && listed) a.l_start[st.ln] = i;
                if (term && !st.dead && listed) a.l_end[st.ln] = i;
                st.dead = st.dead || term;
                if (!st.dead && (st.ln & 3u) == 1u) {               // a content byte of a sequence line
                    const uint32_t u = c | 0x20u;                 // exact membership in {A,C,G,T,a,c,g,t} (mtr_pack_code)
                    unsigned long long e = MTR_FASTA_NO_EVENT;
                    if (!(u == 'a' || u == 'c' || u == 'g' || u == 't')) e = fq_event(i, MTR_FASTA_END_BADCHAR);
                    else if (i - st.ls == (uint32_t)(MTR_MAX_INPUT_LENGTH - 1)) e = fq_event(i, MTR_FASTA_END_TOOLONG);
                    ev = e < ev ? e : ev;
                }
                if (i == (uint32_t)a.n - 1u && !st.dead && listed) a.l_end[st.ln] = (uint32_t)a.n;        // the last line, without a terminator
                if (c == 10u) { st.ln++; st.ls = i + 1u; st.dead = false; }
            }
        }
        fq_post(ev, a.event);
    }
    if (MODE == 1) {
        // first walk: the thread's bases, and where the first of them goes; a tile's bases are neighbours in the text, in file order
        uint32_t nb = 0u, first = 0u;
        {
            FqState st = st0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (j < nv) {
                    const uint32_t c = (x[j >> 2] >> (8 * (j & 3))) & 0xffu, i = (uint32_t)i0 + (uint32_t)j;
                    st.dead = st.dead || fa_is_term(c);
                    if (!st.dead && (st.ln & 3u) == 1u && (st.ln >> 2) < a.n_reads) {
                        if (nb == 0u) first = (uint32_t)a.b_off[st.ln >> 2] + (i - st.ls);
                        nb++;
                    }
                    if (c == 10u) { st.ln++; st.ls = i + 1u; st.dead = false; }
                }
            }
        }
        uint32_t q, nbt;
        fa_block_scan<false, 4>(nb, s, q, nbt);
        if (nb > 0u && q == 0u) s_first = first;                   // (the first thread that has a base)
        FqState st = st0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (j < nv) {
                const uint32_t c = (x[j >> 2] >> (8 * (j & 3))) & 0xffu;
                st.dead = st.dead || fa_is_term(c);
                if (!st.dead && (st.ln & 3u) == 1u && (st.ln >> 2) < a.n_reads && q < MTR_FASTA_TILE_BYTES) s_text[q++] = (uint8_t)c;
                if (c == 10u) { st.ln++; st.dead = false; }
            }
        }
        __syncthreads();
        if (nbt > 0u) {
            const size_t B0 = (size_t)s_first;
            for (uint32_t k = threadIdx.x; k < nbt; k += MTR_FASTA_BLOCK) a.text[B0 + k] = s_text[k];
        }
    }
}

// One thread a record: its four lines against the rules that need the whole line - the stops other than those inside a sequence line -
// and its columns.  A line that does not begin (the file ended) has no entry in the table.
// more: the input goes on behind the buffer - a quality line is checked only if its LF is in the buffer (a line begins behind it, or it
// is the buffer's last byte), and the buffer's end cuts no record.
__global__ __launch_bounds__(256) void mtr_k_fastq_records(FastqArgs a, int32_t more)
{
    unsigned long long ev = MTR_FASTA_NO_EVENT;
    const bool ends_with_lf = more && a.fq[a.n - 1] == (uint8_t)10;
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < a.n_recs; r += gridDim.x * 256u) {
        const uint32_t l = 4u * r;
        unsigned long long e = MTR_FASTA_NO_EVENT, o;
        const uint32_t s0 = a.l_start[l], e0 = a.l_end[l];
        const bool at = e0 > s0 && a.fq[s0] == (uint8_t)'@';
        if (!at) e = fq_event(s0, MTR_FASTA_END_FORMAT);
        uint32_t len = 0u;
        if (l + 1u < a.n_lines) {
            const uint32_t s1 = a.l_start[l + 1u];
            len = a.l_end[l + 1u] - s1;
            if (len == 0u) { o = fq_event(s1, MTR_FASTA_END_EMPTY); e = o < e ? o : e; }
        }
        if (l + 2u < a.n_lines) {
            const uint32_t s2 = a.l_start[l + 2u];
            if (!(a.l_end[l + 2u] > s2 && a.fq[s2] == (uint8_t)'+')) { o = fq_event(s2, MTR_FASTA_END_FORMAT); e = o < e ? o : e; }
        }
        if (l + 3u < a.n_lines) {
            const uint32_t s3 = a.l_start[l + 3u];
            const bool whole = !more || l + 4u < a.n_lines || ends_with_lf;
            if (whole && a.l_end[l + 3u] - s3 != len) { o = fq_event(s3, MTR_FASTA_END_FORMAT); e = o < e ? o : e; }
        } else if (!more) {
            o = fq_event((uint32_t)a.n, MTR_FASTA_END_FORMAT); e = o < e ? o : e;        // the file ends inside the record
        }
        a.r_pos[r] = (int32_t)s0; a.r_idlen[r] = at ? (int32_t)(e0 - s0 - 1u) : 0; a.r_len[r] = (int32_t)len;
        ev = e < ev ? e : ev;
    }
    fq_post(ev, a.event);
}

// The reads before the stop and the sizes.  The stop lies in the record of the line it is on (the end of the file: in the record that
// the file cuts); every record before that one is complete and correct, or the stop would be an earlier one.
// more: the input goes on behind the buffer - without a stop the reads are the records whose fourth LF is in the buffer, and the next
// window starts behind that LF.
__global__ __launch_bounds__(64) void mtr_k_fastq_finish(FastqArgs a, int32_t more, const int64_t *id_off, mtr_fasta_info *info)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long ev = *a.event;
    int32_t n_reads = (int32_t)(a.n_lines >> 2), end = MTR_FASTA_END_EOF, bad = 0; int64_t end_pos = a.n;
    if (ev == MTR_FASTA_NO_EVENT && more) {
        const uint32_t n_lf = a.n_lines - (a.fq[a.n - 1] == (uint8_t)10 ? 0u : 1u);       // (the last line has no LF yet)
        n_reads = (int32_t)(n_lf >> 2); end = MTR_FASTA_END_MORE;
        end_pos = 4u * (uint32_t)n_reads < a.n_lines ? (int64_t)a.l_start[4u * (uint32_t)n_reads] : (int64_t)a.n;
    } else if (ev != MTR_FASTA_NO_EVENT) {
        end = (int32_t)(ev & 7ull); end_pos = (int64_t)(ev >> 3);
        if (end == MTR_FASTA_END_BADCHAR) bad = a.fq[end_pos];
        if (end_pos < (int64_t)a.n) {
            uint32_t lo = 0u, hi = a.n_lines - 1u;                // the last line that starts at or before the stop
            while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if ((int64_t)a.l_start[mid] <= end_pos) lo = mid; else hi = mid - 1u; }
            n_reads = (int32_t)(lo >> 2);
        }
    }
    info->n_reads = n_reads; info->end = end; info->bad_char = bad; info->reserved = 0;
    info->end_pos = end_pos;
    info->n_bases = a.b_off[n_reads];
    info->id_bytes = id_off[n_reads];
}

// offsets[r]: where read r begins in the compacted text (in_file 0: the exclusive sum of the lengths) or in the file itself (in_file 1)
__global__ __launch_bounds__(256) void mtr_k_fastq_reads(FastqArgs a, int32_t n_reads, int32_t in_file, int64_t *offsets, int32_t *lens)
{
    for (int32_t r = (int32_t)(blockIdx.x * 256u + threadIdx.x); r < n_reads; r += (int32_t)(gridDim.x * 256u)) {
        offsets[r] = in_file ? (int64_t)a.l_start[4 * (size_t)r + 1] : a.b_off[r];
        lens[r] = a.r_len[r];
    }
}
