// report_align.hip.inc — mtr_report_alignments_device: mTR's -a alignments of the reported repeats, made and rendered on the device.
//
// The repeats are those of mtr_report_device (chain.hip.inc), repeat k here = repeat k there: the kernels that walk the reads take
// the same RecordView and ChainView.  Per call after a run:
//   mtr_k_align_sizes    one wavefront per read: the path capacity, unit bytes and DP cells its chained repeats need (sums per read,
//                        the largest DP of the batch by one atomic maximum per read);
//   mtr_k_scan_offsets   one workgroup: exclusive prefix sums (per-read capacities and unit bytes; later the path lengths);
//   mtr_k_align_tasks    one wavefront per read: the task columns mtr_k_align takes (AlignArgs), each task's slice of the path and
//                        unit buffers by a wave scan from the read's offset, the unit as base codes;
//   mtr_k_align          (k2_units.hip.inc, unchanged) one wavefront per alignment, the path in TRACEBACK order;
//   mtr_k_align_render   one wavefront per repeat from a work queue, 64 columns a step: the path mirrored into print order and the
//                        three text rows print.c's alignment_block prints.
// A repeat that mtr_alignments would refuse (period outside 1..499, no rows, a window outside the read) becomes a task without
// rows: dp_wrap returns at once and the repeat has zero columns.
//
// Every result is written with ordinary vector stores.

// the task of one reported repeat, as mtr_alignments makes it on the host: window, unit length, path capacity, DP cells
__device__ __forceinline__ void ra_task(const DevRecord *r, int L, int &rs, int &re, int &U, int64_t &cap, int64_t &cells)
{
    rs = r->f[0]; re = r->f[1]; U = r->f[3];
    const int rows = re - rs + 1;
    if (U <= 0 || U >= MTRC_MAX_PERIOD || rows <= 0 || rs < 0 || re > L) { rs = 1; re = 0; U = 0; cap = 0; cells = 0; return; }
    const int g = r->f[10] > 1 ? r->f[10] : 1, d = r->f[12] > 1 ? r->f[12] : 1;
    // columns = rows + deletions; every deletion costs indel_penalty out of a score of at most match_gain per row
    const int64_t max_del = (int64_t)g * (int64_t)rows / (int64_t)d;
    cap = ((int64_t)rows + max_del + (int64_t)U + 64 + 3) & ~(int64_t)3;
    cells = (int64_t)rows * (int64_t)(U + 1);
}

// per read: read_cap[rd] / read_units[rd] = path bytes / unit bytes of its chained repeats; *max_cells = the largest DP of the batch
__global__ void __launch_bounds__(64) mtr_k_align_sizes(RecordView v, ChainView ch, const int32_t *lens,
                                                         int64_t *read_cap, int64_t *read_units, unsigned long long *max_cells)
{
    const int rd = blockIdx.x, lane = threadIdx.x;
    if (rd >= v.n_reads) return;
    const auto [idx, len, k0] = ch.read(rd);
    const DevRecord *src = v.read(rd).rec;
    const int L = lens[rd];
    int64_t cap_sum = 0, unit_sum = 0, cell_max = 0;
    for (int t = lane; t < len; t += 64) {
        int rs, re, U; int64_t cap, cells;
        ra_task(src + idx[t], L, rs, re, U, cap, cells);
        cap_sum += cap; unit_sum += U; cell_max = cells > cell_max ? cells : cell_max;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        cap_sum += __shfl_xor(cap_sum, d); unit_sum += __shfl_xor(unit_sum, d);
        const int64_t o = __shfl_xor(cell_max, d); cell_max = o > cell_max ? o : cell_max;
    }
    if (lane == 0) {
        read_cap[rd] = cap_sum; read_units[rd] = unit_sum;
        if (cell_max > 0) atomicMax(max_cells, (unsigned long long)cell_max);
    }
}

// out[i] = in[0] + .. + in[i - 1] for i = 0 .. n (out[n] = the total): ONE workgroup of 1024, 1024 entries a step - a wave scan, the
// sixteen wave totals through LDS, the steps' total carried in a register
template <typename T>
__global__ void __launch_bounds__(1024) mtr_k_scan_offsets(const T *in, int64_t n, int64_t *out)
{
    __shared__ int64_t s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    for (int64_t c = 0; c < n; c += 1024) {
        const int64_t i = c + tid;
        const int64_t v = i < n ? (int64_t)in[i] : 0;
        int64_t incl = v;
        for (int d = 1; d < 64; d <<= 1) { const int64_t o = __shfl_up(incl, d); if (lane >= d) incl += o; }
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        int64_t before = 0, step = 0;
        for (int k = 0; k < 16; k++) { const int64_t s = s_wave[k]; before += k < w ? s : 0; step += s; }
        if (i < n) out[i] = carry + before + incl - v;
        carry += step;
        __syncthreads();
    }
    if (tid == 0) out[n] = carry;
}

// the columns of AlignArgs for the repeats of read rd (ChainView): their paths from cap_base[rd] on, their units from unit_base[rd] on.
// Lane 0 of read 0 also writes the closing offsets.
struct AlignTaskDst {
    int32_t *read_idx, *rep_start, *rep_end, *gain, *mism, *indel, *unit_off;
    int64_t *ops_off; uint8_t *units; const DevRecord **rec_of;
};
__global__ void __launch_bounds__(64) mtr_k_align_tasks(RecordView v, ChainView ch, const int32_t *lens, const int64_t *cap_base, const int64_t *unit_base,
                                                         int64_t total_repeats, AlignTaskDst o)
{
    const int rd = blockIdx.x, lane = threadIdx.x;
    if (rd >= v.n_reads) return;
    if (rd == 0 && lane == 0) { o.ops_off[total_repeats] = cap_base[v.n_reads]; o.unit_off[total_repeats] = (int32_t)unit_base[v.n_reads]; }
    const auto [idx, len, k0] = ch.read(rd);
    if (len <= 0) return;
    const DevRecord *src = v.read(rd).rec;
    const int L = lens[rd];
    int64_t cbase = cap_base[rd], ubase = unit_base[rd];
    for (int c = 0; c < len; c += 64) {
        const int t = c + lane;
        const DevRecord *r = src;
        int rs = 1, re = 0, U = 0; int64_t cap = 0, cells = 0;
        if (t < len) { r = src + idx[t]; ra_task(r, L, rs, re, U, cap, cells); }
        int64_t cap_incl = cap; int u_incl = U;                              // inclusive scans over the 64 lanes
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t vc = __shfl_up(cap_incl, d); const int vu = __shfl_up(u_incl, d);
            if (lane >= d) { cap_incl += vc; u_incl += vu; }
        }
        if (t < len) {
            const int64_t k = k0 + t, uo = ubase + u_incl - U;
            o.read_idx[k] = rd; o.rep_start[k] = rs; o.rep_end[k] = re; o.gain[k] = r->f[10]; o.mism[k] = r->f[11]; o.indel[k] = r->f[12];
            o.unit_off[k] = (int32_t)uo; o.ops_off[k] = cbase + cap_incl - cap; o.rec_of[k] = r;
            for (int b = 0; b < U; b++) { const char ch = r->unit[b]; o.units[uo + b] = (uint8_t)(ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3); }
        }
        cbase += __shfl(cap_incl, 63); ubase += __shfl(u_incl, 63);
    }
}

// What mtr_k_align left (traceback order) and where the rendered columns go (print order).
struct AlignRenderArgs {
    BatchView b;
    int32_t n_repeats;
    const int32_t *read_idx, *rep_start, *ops_len, *ends;       // ends as AlignArgs: [2k] row in the window, [2k+1] unit column of the path's last cell
    const uint8_t *path; const int64_t *path_off;               // repeat k's path = path[path_off[k] .. + ops_len[k])
    const DevRecord *const *rec_of;
    const int64_t *col_off; int64_t n_columns;                  // columns of repeat k = col_off[k] .. col_off[k + 1] of n_columns
    uint8_t *ops, *text; int32_t *first;
    unsigned int *work_counter;
};

// One alignment as the kernels that print it see it: repeat k's path in traceback order and what its columns are read from.
struct AlignCols {
    const uint8_t *path; const uint32_t *pk; const DevRecord *r;
    int n, U, L, end_pos, end_col;
    int used_p, used_j;                                              // read bases / unit columns the steps before this one consumed
};
// false: alignment_block prints only the scores line (no columns, or no unit).  Wave-uniform.
__device__ __forceinline__ bool align_cols_begin(AlignCols &s, const AlignRenderArgs &a, int k)
{
    s.n = uni(a.ops_len[k]);
    s.r = (const DevRecord *)uni64((long long)a.rec_of[k]);
    s.U = uni(s.r->f[3]);
    if (s.n <= 0 || s.U <= 0) return false;
    const int rd = uni(a.read_idx[k]);
    s.pk = a.b.packed + uni64(a.b.woff[rd]);
    s.L = uni(a.b.lens[rd]);
    s.end_pos = uni(a.rep_start[k]) - 1 + uni(a.ends[2 * k]); s.end_col = uni(a.ends[2 * k + 1]);
    s.path = a.path + uni64(a.path_off[k]);
    s.used_p = 0; s.used_j = 0;
    return true;
}
// One step of 64 columns.  Column q = c + lane of the path (q = 0: the LAST printed column) shows read position
// p(q) = end_pos - #{q' < q : no gap in the read} and unit column j(q) = ((end_col - 1 - #{q' < q : no gap in the unit}) mod U) + 1:
// two ballots and the count of the lanes below per step, the steps' totals carried in s.  Returns q < n; then op is the column's
// operation, p its read position, x its 0-origin unit column and row[0 .. 3) the three characters alignment_block prints for it.
__device__ __forceinline__ bool align_cols_step(AlignCols &s, int c, int &op, int &p, int &x, uint8_t row[3])
{
    const int q = c + lane_id();
    const bool in = q < s.n;
    op = in ? (int)s.path[q] : 0;
    const unsigned long long mp = __ballot(in && op != 3), mj = __ballot(in && op != 4);
    p = s.end_pos - s.used_p - mbcnt(mp);
    x = (s.end_col - 1 - s.used_j - mbcnt(mj)) % s.U;
    if (x < 0) x += s.U;
    if (in) {
        // positions L and L + 1 read what the image holds there (zero, or in file-order mode the bases an earlier read left): the bits the DP saw
        const int code = (p >= 0 && p < s.L + 2) ? base_at(s.pk, p) : 0;
        const uint8_t xb = (uint8_t)(0x54474341u >> (8 * code)), ub = (uint8_t)s.r->unit[x];      // "ACGT"
        row[0] = op == 3 ? (uint8_t)'-' : xb;
        row[1] = op == 1 ? (uint8_t)'|' : (uint8_t)' ';
        row[2] = op == 4 ? (uint8_t)'-' : ub;
    }
    s.used_p += __popcll(mp); s.used_j += __popcll(mj);
    return in;
}

// One wavefront per repeat, 64 columns a step (align_cols_step).  Lane q writes index n - 1 - q: the path mirrored into print order.
__global__ void __launch_bounds__(64) mtr_k_align_render(AlignRenderArgs a)
{
    const int lane = lane_id();
    for (;;) {
        const int k = next_work_item(a.work_counter);
        if (k >= a.n_repeats) break;                                  // every wave reaches this exit
        AlignCols s;
        if (!align_cols_begin(s, a, k)) {                             // alignment_block prints only the scores line
            if (lane == 0) { a.first[2 * k] = 0; a.first[2 * k + 1] = 0; }
            loop_join();
            continue;
        }
        const int n = s.n;
        const int64_t o0 = uni64(a.col_off[k]) + (int64_t)(n - 1), C = a.n_columns;
        for (int c = 0; c < n; c += 64) {
            int op, p, x; uint8_t row[3];
            if (align_cols_step(s, c, op, p, x, row)) {
                const int q = c + lane;
                const int64_t o = o0 - q;
                a.ops[o] = (uint8_t)op;
                a.text[o] = row[0];
                a.text[C + o] = row[1];
                a.text[2 * C + o] = row[2];
                if (q == n - 1) { a.first[2 * k] = p; a.first[2 * k + 1] = x + 1; }
            }
        }
        loop_join();
    }
}
