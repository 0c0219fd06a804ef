// chain.hip.inc — mtr_report_device: mTR's report on the device.  Per read the maximum-score chain of its records
// (reference chaining.cpp:243-363), index for index what mtr_amd/host/chain.c (mtrh_chain) returns, then the chained
// repeats written out as columns.
//
// mtr_k_chain: one wavefront per read runs the reference's sweep.
//   - Each record i with rep_start + 10 <= rep_end gives a start event (key rep_start) and an end event (key rep_end - 10).
//     Ordering events by (key, creation sequence) is ordering them by (key, record, start before end), so every lane ranks
//     its events by counting the smaller ones and scatters them to their place: no sort network, any count.
//   - The sweep over the events is serial by nature; Y (the chain ends found so far, ordered by end, ties in insertion
//     order) is scanned 64 entries a step with ballots: the predecessor and "a better one exists" are prefix counts (Y is
//     sorted, so the prefix with end <= x is a count); an end event rebuilds Y into the other of two buffers with the new
//     entry inserted, applying the reference's erase loop (chaining.cpp:316-328) as a scalar walk over the erase mask:
//     take bit t, go on at t + 2 (the element behind an erased one is skipped), carried across the 64-entry steps.
//   - The chain is the predecessor walk from the last element of Y (lane 0, serial).
//   Working arrays: 12 n + 6 ints for n records.  Reads of up to MTR_CHAIN_LDS_RECS records (nearly all: config 4 averages
//   2.7) keep them in LDS; longer reads in per-read global scratch the host lays out (any count).
// mtr_k_report_pack: one wavefront per read writes its chained repeats at the read's offset into the caller's columns.
// The records come through a RecordView (records.hip.inc); what mtr_k_chain found, every later kernel of the report reads through
// a ChainView: the chain of read rd and the number of its first repeat.
//
// Every result is written with ordinary vector stores.

#define MTR_CHAIN_OVERLAP 10                                   // MAX_LEN_overlapping (reference mTR.h:39)
#define MTR_CHAIN_LDS_RECS 192                                 // 12 x 192 + 6 ints = 9 240 bytes of LDS per wavefront
#define MTR_CHAIN_INTS(n) (12 * (int64_t)(n) + 6)

__device__ __forceinline__ int chain_lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ int chain_unit_len(const DevRecord *r)
{   // strnlen(unit, period): what print.c's report_line prints
    const int p = r->f[3] < 0 ? 0 : (r->f[3] > MTRC_MAX_PERIOD ? MTRC_MAX_PERIOD : r->f[3]);
    int n = 0;
    while (n < p && r->unit[n]) n++;
    return n;
}

// the printed "match ratio": (float)num_matches / repeat_len, the ratio column of mtr_report_device and the float mtr_report_text_device prints
__device__ __forceinline__ float report_ratio(int matches, int repeat_len)
{
    float ratio = (float)matches / (float)repeat_len;                // correctly rounded (build.py), as the host's float division
    if (ratio != ratio) ratio = __int_as_float((int)0xffc00000u);    // 0 / 0: the NaN an x86 host makes (printed "-nan")
    return ratio;
}

// the records of a read: DevRecord slots (the product) or caller-given triples (mtr_test_chain)
struct ChainRecs {
    const DevRecord *rec;                                      // non-null: f[0] start, f[1] end, f[5] matches
    const int32_t *start, *end, *matches;                      // else: plain arrays
    __device__ __forceinline__ void get(int i, int &s, int &e, int &m) const
    {
        if (rec) { s = rec[i].f[0]; e = rec[i].f[1]; m = rec[i].f[5]; }
        else { s = start[i]; e = end[i]; m = matches[i]; }
    }
};

// The sweep of chain.c for one read of n records (all 64 lanes call it); the chain goes to out[0 .. len), print order.
// mem: 12 n + 6 ints of LDS or global memory.  Returns len (every lane).
__device__ int chain_one_read(const ChainRecs &src, int n, int *mem, int32_t *out)
{
    const int lane = threadIdx.x;
    if (n <= 0) return 0;
    if (n == 1) {                                              // a lone record is its own chain iff it enters the sweep at all
        int s, e, m; src.get(0, s, e, m);
        const int len = s + MTR_CHAIN_OVERLAP <= e ? 1 : 0;
        if (len && lane == 0) out[0] = 0;
        return len;
    }
    const int S = n + 1;
    int *rs = mem, *re = rs + n, *sc = re + n, *pred = sc + n, *ev = pred + n;
    int *const yb = ev + 2 * n;                                 // Y in two buffers b = 0, 1: ends at yb + b S, scores + (2 + b) S, records + (4 + b) S
    int n_part = 0;
    for (int i = lane; i - lane < n; i += 64) {
        int s = 0, e = 0, m = 0;
        if (i < n) { src.get(i, s, e, m); rs[i] = s; re[i] = e; sc[i] = m; pred[i] = -1; }
        n_part += __popcll(__ballot(i < n && s + MTR_CHAIN_OVERLAP <= e));
    }
    __syncthreads();
    // rank = number of events before this one in (key, record, kind) order = (key, creation sequence) order
    for (int i = lane; i < n; i += 64) {
        const int s = rs[i], e = re[i];
        if (s + MTR_CHAIN_OVERLAP > e) continue;
        const int64_t k0 = ((int64_t)s * 4294967296ll) | (uint32_t)(2 * i), k1 = ((int64_t)(e - MTR_CHAIN_OVERLAP) * 4294967296ll) | (uint32_t)(2 * i + 1);
        int r0 = 0, r1 = 0;
        for (int j = 0; j < n; j++) {
            const int sj = rs[j], ej = re[j];
            if (sj + MTR_CHAIN_OVERLAP > ej) continue;
            const int64_t j0 = ((int64_t)sj * 4294967296ll) | (uint32_t)(2 * j), j1 = ((int64_t)(ej - MTR_CHAIN_OVERLAP) * 4294967296ll) | (uint32_t)(2 * j + 1);
            r0 += (j0 < k0) + (j1 < k0);
            r1 += (j0 < k1) + (j1 < k1);
        }
        ev[r0] = 2 * i; ev[r1] = 2 * i + 1;
    }
    __syncthreads();
    const int n_ev = 2 * n_part;
    int ny = 0, cur = 0;
    for (int x = 0; x < n_ev; x++) {
        const int v = ev[x], a = v >> 1, rsa = rs[a], rea = re[a];
        if ((v & 1) == 0 || rea - MTR_CHAIN_OVERLAP == rsa) {                       // Alignment::isStart: the key equals the start
            const int lim = rsa + MTR_CHAIN_OVERLAP;
            int cnt = 0;                                                            // Y is sorted by end: the last one within lim is entry cnt - 1
            for (int c = 0; c < ny; c += 64) {
                const int t = c + lane;
                const unsigned long long in = __ballot(t < ny), le = __ballot(t < ny && yb[cur * S + t] <= lim);
                cnt += __popcll(le);
                if (le != in) break;
            }
            if (cnt > 0) {
                const int p = yb[(4 + cur) * S + cnt - 1], ps = yb[(2 + cur) * S + cnt - 1];
                if (lane == 0) { pred[a] = p; sc[a] += ps; }
            }
            __syncthreads();
            continue;
        }
        const int sca = sc[a];
        int pos = 0; bool better = false;
        for (int c = 0; c < ny; c += 64) {
            const int t = c + lane;
            const bool le = t < ny && yb[cur * S + t] <= rea;
            const unsigned long long in = __ballot(t < ny), lem = __ballot(le);
            better = better || __ballot(le && yb[(2 + cur) * S + t] > sca) != 0ull;
            pos += __popcll(lem);
            if (lem != in) break;
        }
        if (better) continue;
        // Y' = Y with a inserted at pos; every y with end >= end(a) and a lower score is erased, skipping the one behind
        const int m = ny + 1, nxt = cur ^ 1;
        int out_n = 0; bool skip = false;
        for (int c = 0; c < m; c += 64) {
            const int t = c + lane;
            int e = 0, s = 0, id = 0;
            if (t < m) {
                if (t < pos) { e = yb[cur * S + t]; s = yb[(2 + cur) * S + t]; id = yb[(4 + cur) * S + t]; }
                else if (t == pos) { e = rea; s = sca; id = a; }
                else { e = yb[cur * S + t - 1]; s = yb[(2 + cur) * S + t - 1]; id = yb[(4 + cur) * S + t - 1]; }
            }
            unsigned long long mm = __ballot(t < m && e >= rea && s < sca), erased = 0ull;
            if (skip) mm &= ~1ull;
            skip = false;
            while (mm) {
                const int b = __builtin_ctzll(mm);
                erased |= 1ull << b;
                if (b == 63) skip = true;
                mm &= ~(3ull << b);
            }
            const bool keep = t < m && !((erased >> lane) & 1ull);
            const unsigned long long km = __ballot(keep);
            if (keep) { const int o = out_n + chain_lanes_below(km); yb[nxt * S + o] = e; yb[(2 + nxt) * S + o] = s; yb[(4 + nxt) * S + o] = id; }
            out_n += __popcll(km);
        }
        ny = out_n; cur = nxt;
        __syncthreads();
    }
    int len = 0;
    if (ny > 0) {
        if (lane == 0) {
            const int last = yb[(4 + cur) * S + ny - 1];
            for (int q = last; q >= 0; q = pred[q]) len++;
            int p = len;
            for (int q = last; q >= 0; q = pred[q]) out[--p] = q;
        }
        len = __shfl(len, 0);
    }
    return len;
}

// per read: chain_idx[rec_off[rd] ..] = the chain (record indices, print order), chain_len[rd], unit_bytes[rd] = the bytes of
// its repeats' units.  scr_off[rd] >= 0: the read's working arrays are scratch + scr_off[rd] (more than MTR_CHAIN_LDS_RECS records).
__global__ void __launch_bounds__(64) mtr_k_chain(RecordView v, const int64_t *rec_off, const int64_t *scr_off, int32_t *scratch, int32_t *chain_idx,
                                                   int32_t *chain_len, int32_t *unit_bytes)
{
    __shared__ int lds[MTR_CHAIN_INTS(MTR_CHAIN_LDS_RECS)];
    const int rd = blockIdx.x;
    if (rd >= v.n_reads) return;
    const auto [src, c] = v.read(rd);
    int *mem = c <= MTR_CHAIN_LDS_RECS ? lds : scratch + scr_off[rd];
    ChainRecs r = { src, nullptr, nullptr, nullptr };
    int32_t *out = chain_idx + rec_off[rd];
    const int len = chain_one_read(r, c, mem, out);
    __syncthreads();
    int ub = 0;
    for (int t = threadIdx.x; t < len; t += 64) ub += chain_unit_len(src + out[t]);
    for (int d = 32; d >= 1; d >>= 1) ub += __shfl_xor(ub, d);
    if (threadIdx.x == 0) { chain_len[rd] = len; unit_bytes[rd] = ub; }
}

// mtr_test_chain: set k = triples set_off[k] .. set_off[k+1]; its chain at chain_idx[set_off[k] ..]
__global__ void __launch_bounds__(64) mtr_k_chain_sets(const int32_t *start, const int32_t *end, const int32_t *matches, const int64_t *set_off, int n_sets,
                                                        const int64_t *scr_off, int32_t *scratch, int32_t *chain_idx, int32_t *chain_len)
{
    __shared__ int lds[MTR_CHAIN_INTS(MTR_CHAIN_LDS_RECS)];
    const int k = blockIdx.x;
    if (k >= n_sets) return;
    const int64_t o = set_off[k];
    const int n = (int)(set_off[k + 1] - o);
    int *mem = n <= MTR_CHAIN_LDS_RECS ? lds : scratch + scr_off[k];
    ChainRecs r = { nullptr, start + o, end + o, matches + o };
    const int len = chain_one_read(r, n, mem, chain_idx + o);
    if (threadIdx.x == 0) chain_len[k] = len;
}

// What mtr_k_chain left: read rd's chain is chain_idx[rec_off[rd] .. + chain_len[rd]), its repeats are k = rep_off[rd] .. + chain_len[rd]
struct ReadChain { const int32_t *idx; int len; int64_t k0; };
struct ChainView {
    const int64_t *rec_off; const int32_t *chain_idx, *chain_len; const int64_t *rep_off;
    __device__ __forceinline__ ReadChain read(int rd) const { return { chain_idx + rec_off[rd], chain_len[rd], rep_off[rd] }; }
};

// Columns of mtr_report_dst for read rd: its repeats (ChainView), their units from unit_base[rd] on.
// Lane 0 of read 0 also writes unit_off[total_repeats] = total_unit_bytes.
__global__ void __launch_bounds__(64) mtr_k_report_pack(RecordView v, ChainView ch, const int64_t *unit_base, int64_t total_repeats, int64_t total_unit_bytes,
                                                         int32_t *o_read, int32_t *o_record, int32_t *o_fields, float *o_ratio, int64_t *o_unit_off, uint8_t *o_units)
{
    const int rd = blockIdx.x, lane = threadIdx.x;
    if (rd >= v.n_reads) return;
    if (rd == 0 && lane == 0) o_unit_off[total_repeats] = total_unit_bytes;
    const auto [idx, len, k0] = ch.read(rd);
    if (len <= 0) return;
    const DevRecord *src = v.read(rd).rec;
    for (int q = lane; q < 14 * len; q += 64) {
        const int t = q / 14, f = q - 14 * t;
        o_fields[(k0 + t) * 14 + f] = src[idx[t]].f[f];
    }
    int64_t ubase = unit_base[rd];
    for (int c = 0; c < len; c += 64) {
        const int t = c + lane;
        int ul = 0, i = 0;
        if (t < len) {
            i = idx[t];
            const DevRecord *r = src + i;
            ul = chain_unit_len(r);
            o_read[k0 + t] = rd; o_record[k0 + t] = i;
            o_ratio[k0 + t] = report_ratio(r->f[5], r->f[2]);
        }
        int incl = ul;                                                       // inclusive scan of the unit lengths over the 64 lanes
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d); if (lane >= d) incl += v; }
        const int64_t uo = ubase + incl - ul;
        if (t < len) {
            o_unit_off[k0 + t] = uo;
            for (int b = 0; b < ul; b++) o_units[uo + b] = (uint8_t)src[i].unit[b];
        }
        ubase += __shfl(incl, 63);
    }
}
