// report_text.hip.inc — mtr_report_text_device: the bytes mTR writes to stdout for the resident batch, -a too, formatted on the device.
//
// The repeats are those of mtr_report_device (chain.hip.inc) and, with alignments, the paths mtr_report_alignments_device keeps
// (report_align.hip.inc); TextArgs carries the same RecordView and ChainView.  Per call:
//   mtr_k_text_lines<false>  one wavefront per read, a lane per repeat: the exact byte count of each repeat's output;
//   mtr_k_scan_offsets       (report_align.hip.inc) the repeats' byte offsets; read i's section starts at the offset of its first repeat;
//   mtr_k_text_lines<true>   the same walk again, writing: the report line of print.c's report_line, with alignments the scores line of
//                            alignment_block, the read offsets, and where each repeat's alignment rows begin;
//   mtr_k_text_align         one wavefront per repeat from a work queue, 64 columns a step (align_cols_step, shared with
//                            mtr_k_align_render): every column's three characters straight to their place in the byte stream.
// Sizes and contents come from ONE set of functions, templated on WRITE: the size pass runs them with WRITE = false, so a count can
// not disagree with what is written later.
//
// Layout of one repeat:  ID \t L \t start+1 \t end+1 \t repeat_len \t period \t copies \t matches \t ratio \t mismatches \t insertions
// \t deletions \t unit \n   and with alignments   \n "match gain = G, mismatch penalty = M, indel penalty = D" \n \n   then, for n
// columns, blocks of MTR_TEXT_ALIGN_WIDTH: block b = print-order columns 50 b .. 50 b + w (w = 50, the last one n - 50 b) is
// row 0 \n row 1 \n row 2 \n \n = 3 w + 4 bytes, so block b starts 154 b bytes into the rows and column i = 50 b + x of row r is byte
// 154 b + r (w + 1) + x.  In all 3 n + 4 ceil(n / 50) bytes; a repeat without columns has the scores line only.
//
// The ratio is printf("%f") of the float (float)num_matches / repeat_len (report_ratio: bit for bit the ratio column of
// mtr_report_device), by the integer method of print.c's mtrh_format_ratio: the 24-bit significand times 10^6 is exact in 44 bits,
// shifted by the exponent, rounded half to even on the exact remainder - what a correctly rounded printf prints.  A quotient of two
// int32 is at most 2^31 in magnitude, so the shifted value fits 64 bits: no other path exists.  A set sign bit prints '-' (negative
// values, -0.000000); infinities print inf / -inf; a NaN prints nan / -nan by the sign bit of the float the device made, exactly as
// format_report prints the ratio column.  report_ratio gives 0 / 0 the NaN an x86 host makes, so it prints -nan as print.c does there
// (printf of an x86 host's 0.0f / 0).  No record the kernels make has repeat_len 0: the case exists for mtr_test_report_lines.
//
// Every result is written with ordinary vector stores.

#define MTR_TEXT_ALIGN_WIDTH 50                                // ALIGNMENT_WIDTH_PRINTING (reference mTR.h:38), MTRH_ALIGN_WIDTH of the host
#define MTR_TEXT_BLOCK_BYTES (3 * MTR_TEXT_ALIGN_WIDTH + 4)

// "%d" as print.c's put_int (INT_MIN too: the magnitude is taken unsigned); returns the characters
template <bool WRITE>
__device__ __forceinline__ int rt_put_int(uint8_t *o, int64_t at, int v)
{
    unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    const int neg = v < 0 ? 1 : 0;
    int nd = 1;
    for (unsigned t = u; t >= 10u; t /= 10u) nd++;
    if (WRITE) {
        if (neg) o[at] = (uint8_t)'-';
        for (int d = neg + nd - 1; d >= neg; d--) { o[at + d] = (uint8_t)('0' + u % 10u); u /= 10u; }
    }
    return neg + nd;
}

// "%f" of f, |f| <= 2^31 or not finite (the header of this file); returns the characters
template <bool WRITE>
__device__ __forceinline__ int rt_put_ratio(uint8_t *o, int64_t at, float f)
{
    const uint32_t bits = (uint32_t)__float_as_int(f);
    const int ex = (int)((bits >> 23) & 0xffu);
    int n = 0;
    if (bits >> 31) { if (WRITE) o[at] = (uint8_t)'-'; n = 1; }
    if (ex == 255) {
        if (WRITE) {
            const bool nan = (bits & 0x7fffffu) != 0u;
            o[at + n] = (uint8_t)(nan ? 'n' : 'i'); o[at + n + 1] = (uint8_t)(nan ? 'a' : 'n'); o[at + n + 2] = (uint8_t)(nan ? 'n' : 'f');
        }
        return n + 3;
    }
    uint64_t q = 0;                                            // the magnitude x 10^6, rounded (zero and subnormals: below 10^-37)
    if (ex != 0) {
        const uint64_t N = (uint64_t)((bits & 0x7fffffu) | 0x800000u) * 1000000ull;     // below 2^44
        const int e = ex - 150;                                // magnitude = M x 2^e; e <= 8 for |f| <= 2^31
        if (e >= 0) q = N << (e < 19 ? e : 19);
        else if (-e <= 62) {
            const int s = -e;
            const uint64_t rem = N & ((1ull << s) - 1ull), half = 1ull << (s - 1);
            q = N >> s;
            if (rem > half || (rem == half && (q & 1ull))) q++;
        }
    }
    uint64_t ip = q / 1000000ull; unsigned fr = (unsigned)(q % 1000000ull);
    int nd = 1;
    for (uint64_t t = ip; t >= 10ull; t /= 10ull) nd++;
    if (WRITE) {
        for (int d = n + nd - 1; d >= n; d--) { o[at + d] = (uint8_t)('0' + (unsigned)(ip % 10ull)); ip /= 10ull; }
        o[at + n + nd] = (uint8_t)'.';
        for (int d = 6; d >= 1; d--) { o[at + n + nd + d] = (uint8_t)('0' + fr % 10u); fr /= 10u; }
    }
    return n + nd + 7;
}

template <bool WRITE>
__device__ __forceinline__ int rt_put_str(uint8_t *o, int64_t at, const char *s, int n)
{
    if (WRITE) for (int b = 0; b < n; b++) o[at + b] = (uint8_t)s[b];
    return n;
}

// print.c's report_line for one repeat: f = the 14 header ints, unit[0 .. ulen) what is printed of the unit.  Returns the bytes.
template <bool WRITE>
__device__ __forceinline__ int64_t rt_line(uint8_t *o, int64_t at, const uint8_t *id, int64_t id_len, int L, const int32_t *f, const char *unit, int ulen)
{
    int64_t n = at;
    if (WRITE) for (int64_t b = 0; b < id_len; b++) o[n + b] = id[b];
    n += id_len;
#define RT_TAB() do { if (WRITE) o[n] = (uint8_t)'\t'; n++; } while (0)
    RT_TAB(); n += rt_put_int<WRITE>(o, n, L);
    RT_TAB(); n += rt_put_int<WRITE>(o, n, (int)((unsigned)f[0] + 1u));
    RT_TAB(); n += rt_put_int<WRITE>(o, n, (int)((unsigned)f[1] + 1u));
    RT_TAB(); n += rt_put_int<WRITE>(o, n, f[2]);
    RT_TAB(); n += rt_put_int<WRITE>(o, n, f[3]);
    RT_TAB(); n += rt_put_int<WRITE>(o, n, f[4]);
    RT_TAB(); n += rt_put_int<WRITE>(o, n, f[5]);
    RT_TAB(); n += rt_put_ratio<WRITE>(o, n, report_ratio(f[5], f[2]));
    RT_TAB(); n += rt_put_int<WRITE>(o, n, f[6]);
    RT_TAB(); n += rt_put_int<WRITE>(o, n, f[7]);
    RT_TAB(); n += rt_put_int<WRITE>(o, n, f[8]);
    RT_TAB();
#undef RT_TAB
    if (WRITE) for (int b = 0; b < ulen; b++) o[n + b] = (uint8_t)unit[b];
    n += ulen;
    if (WRITE) o[n] = (uint8_t)'\n';
    return n + 1 - at;
}

// what alignment_block prints in front of the rows: an empty line, the scores, an empty line.  Returns the bytes.
template <bool WRITE>
__device__ __forceinline__ int rt_scores(uint8_t *o, int64_t at, const int32_t *f)
{
    int64_t n = at;
    n += rt_put_str<WRITE>(o, n, "\nmatch gain = ", 14);
    n += rt_put_int<WRITE>(o, n, f[10]);
    n += rt_put_str<WRITE>(o, n, ", mismatch penalty = ", 21);
    n += rt_put_int<WRITE>(o, n, f[11]);
    n += rt_put_str<WRITE>(o, n, ", indel penalty = ", 18);
    n += rt_put_int<WRITE>(o, n, f[12]);
    n += rt_put_str<WRITE>(o, n, "\n\n", 2);
    return (int)(n - at);
}

// the rows of n columns: three rows and an empty line per block of MTR_TEXT_ALIGN_WIDTH
__device__ __forceinline__ int64_t rt_rows_bytes(int n, int U)
{
    if (n <= 0 || U <= 0) return 0;                            // as align_cols_begin: only the scores line
    return 3 * (int64_t)n + 4 * (int64_t)((n + MTR_TEXT_ALIGN_WIDTH - 1) / MTR_TEXT_ALIGN_WIDTH);
}

struct TextArgs {
    RecordView v; ChainView ch; const int32_t *lens;            // the records, the chains, the reads' lengths
    int64_t total_repeats;
    const uint8_t *ids; const int64_t *id_off;                  // read i's ID = ids[id_off[i] .. id_off[i + 1])
    const int32_t *ops_len;                                     // with alignments: the columns of every repeat; else null
    int64_t *bytes;                                             // WRITE = false: [R] the bytes of every repeat's output
    const int64_t *byte_off;                                    // WRITE = true: [R + 1] their exclusive prefix sums
    uint8_t *text; int64_t *read_off, *rows_off;                // WRITE = true: the stream, the reads' offsets (or null), [R] where each repeat's rows begin
};

// One wavefront per read, a lane per repeat of its chain.
template <bool WRITE>
__global__ void __launch_bounds__(64) mtr_k_text_lines(TextArgs a)
{
    const int rd = blockIdx.x, lane = threadIdx.x;
    if (rd >= a.v.n_reads) return;
    const auto [idx, len, k0] = a.ch.read(rd);
    if (WRITE && a.read_off && lane == 0) {
        a.read_off[rd] = a.byte_off[k0];
        if (rd == 0) a.read_off[a.v.n_reads] = a.byte_off[a.total_repeats];
    }
    if (len <= 0) return;
    const DevRecord *src = a.v.read(rd).rec;
    const int L = a.lens[rd];
    const int64_t i0 = a.id_off[rd], id_len = a.id_off[rd + 1] - i0;
    for (int t = lane; t < len; t += 64) {
        const DevRecord *r = src + idx[t];
        const int64_t k = k0 + t, at = WRITE ? a.byte_off[k] : 0;
        int64_t n = rt_line<WRITE>(a.text, at, a.ids + i0, id_len, L, r->f, r->unit, chain_unit_len(r));
        if (a.ops_len) {
            n += rt_scores<WRITE>(a.text, at + n, r->f);
            if (WRITE) a.rows_off[k] = at + n;
            n += rt_rows_bytes(a.ops_len[k], r->f[3]);
        }
        if (!WRITE) a.bytes[k] = n;
    }
}

// mtr_test_report_lines: rt_line on caller-given rows, a lane per row.  Row k: fields[14 k ..], read_len[k], its unit
// units[unit_off[k] .. unit_off[k + 1]) and its ID; its line goes to text[byte_off[k] ..] (WRITE) or its size to bytes[k].
template <bool WRITE>
__global__ void __launch_bounds__(64) mtr_k_text_rows(int n_rows, const int32_t *fields, const int32_t *read_len, const uint8_t *units, const int64_t *unit_off,
                                                       const uint8_t *ids, const int64_t *id_off, int64_t *bytes, const int64_t *byte_off, uint8_t *text)
{
    const int k = (int)(blockIdx.x * 64u + threadIdx.x);
    if (k >= n_rows) return;
    const int64_t u0 = unit_off[k], i0 = id_off[k];
    const int64_t n = rt_line<WRITE>(text, WRITE ? byte_off[k] : 0, ids + i0, id_off[k + 1] - i0, read_len[k], fields + 14 * (size_t)k,
                                     (const char *)units + u0, (int)(unit_off[k + 1] - u0));
    if (!WRITE) bytes[k] = n;
}

// One wavefront per repeat from the work queue, 64 columns a step.  Lane q of a step holds path column q (print-order column
// i = n - 1 - q) and stores its three characters; the lane of a block's last column also stores the block's four line ends.
__global__ void __launch_bounds__(64) mtr_k_text_align(AlignRenderArgs a, const int64_t *rows_off, uint8_t *text)
{
    const int lane = lane_id();
    for (;;) {
        const int k = next_work_item(a.work_counter);
        if (k >= a.n_repeats) break;                                  // every wave reaches this exit
        AlignCols s;
        if (!align_cols_begin(s, a, k)) { loop_join(); continue; }
        const int n = s.n;
        uint8_t *const o = text + uni64(rows_off[k]);
        for (int c = 0; c < n; c += 64) {
            int op, p, x; uint8_t row[3];
            if (align_cols_step(s, c, op, p, x, row)) {
                const int i = n - 1 - (c + lane), b = i / MTR_TEXT_ALIGN_WIDTH, col = i - b * MTR_TEXT_ALIGN_WIDTH;
                const int left = n - b * MTR_TEXT_ALIGN_WIDTH, w = left < MTR_TEXT_ALIGN_WIDTH ? left : MTR_TEXT_ALIGN_WIDTH;
                uint8_t *const blk = o + (int64_t)b * MTR_TEXT_BLOCK_BYTES;
                blk[col] = row[0]; blk[w + 1 + col] = row[1]; blk[2 * (w + 1) + col] = row[2];
                if (col == w - 1) { blk[w] = (uint8_t)'\n'; blk[2 * w + 1] = (uint8_t)'\n'; blk[3 * w + 2] = (uint8_t)'\n'; blk[3 * w + 3] = (uint8_t)'\n'; }
            }
        }
        loop_join();
    }
}
