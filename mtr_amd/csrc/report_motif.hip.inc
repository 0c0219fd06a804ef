// report_motif.hip.inc — mtr_report_motifs_device: the motif catalogue of the reported repeats, made on the device.
//
// The repeats are those of mtr_report_device (chain.hip.inc), repeat k here = repeat k there.  A repeat's unit is printed in whatever
// phase and strand the read had; unit_motif() (unit_motif.h, the single definition) gives its canonical motif, and the kernels here
// group the repeats of a batch by motif.  Per batch, on first use after a run:
//   mtr_k_unit_motif     one workgroup of 64 per read (RecordView, ChainView), MOTIF_TILE of its repeats a step: the units are staged
//                        in LDS, 8 bytes a lane a load (a DevRecord's unit starts on an 8-byte boundary), then two lanes per unit run
//                        unit_motif() on its copy: one strand's least rotation each, the even lane the rest.  Repeat k gets strand, rotation, motif_len, the motif's hash, its motif bytes at the
//                        unit's offset of mtr_report_device (a motif is never longer than its unit), and what the aggregation adds;
//   mtr_k_unit_motif_rows  the same on caller-given units (mtr_test_unit_motifs), MOTIF_TILE rows per workgroup;
//   mtr_k_motif_insert   a lane per repeat, an open-addressing table of uint32 slots (a power of two, at least 2R): from the hash's
//                        start slot, old = atomicCAS(slot, EMPTY, k); EMPTY: in; else the motifs of old and k are compared byte for byte
//                        (the kernel before wrote them: plain loads) - equal: atomicMin(slot, k), done; different: the next slot.  A
//                        slot never changes its motif, so all repeats of a motif end on one slot, which holds their smallest index
//                        when the kernel has finished.  Every access to the table is an agent-scope atomic;
//   mtr_k_motif_leader   (the NEXT kernel: the table is final) leader[k] = its slot's value; first[k] = (leader[k] == k), and the motif
//                        length of such a first repeat;
//   mtr_k_scan_offsets   (report_align.hip.inc) twice: the exclusive sums of first[] = the group numbers, in the order of the groups'
//                        first repeats, and of the first repeats' motif lengths = motif_off;
//   mtr_k_motif_groups   a lane per repeat: group[k]; a group's first repeat writes g_first, motif_off and the motif's bytes; the
//                        members add to g_repeats, g_reads, g_copies, g_bases with integer atomicAdd only - the sums do not depend on
//                        the schedule - after the lanes of a wavefront that share a group have added up among themselves (one atomic
//                        per group and wavefront and column).  For g_reads a repeat counts iff no earlier repeat of its read has its
//                        group (the walk back over the read's repeats stops at the first one found).
// Every result is written with ordinary vector stores.

#include "unit_motif.h"

#define MOTIF_TILE 16                                    // units staged per step: 16 x 512 bytes of LDS
#define MOTIF_SLOT_BYTES 512                             // MTRC_MAX_PERIOD + 4 bytes of unit, padded
#define MOTIF_EMPTY 0xFFFFFFFFu

// per repeat, in buffers of the context: what mtr_k_unit_motif leaves for the grouping
struct MotifRows {
    uint8_t *strand; int32_t *rotation, *motif_len, *read, *bases; int64_t *copies; unsigned long long *hash;
    int64_t *unit_off;                                   // [n + 1]: repeat k's motif is motif[unit_off[k] .. + motif_len[k])
    uint8_t *motif;
};

// Lanes 2t and 2t + 1 work on unit t of a tile (on: the tile has a unit t), p bytes at u (LDS): each walks one strand to its least rotation,
// the even lane does the rest - unit_motif() with its two walks side by side - and writes row k: copies = num_freq_unit x (p / motif_len),
// 0 for an empty unit.  Every lane of the wavefront calls it.
__device__ __forceinline__ void motif_row(const uint8_t *u, int p, bool on, int lane, int64_t k, int64_t uo, int rd, int nfu, int rep_len, const MotifRows &o)
{
    const int r = on && p > 0 ? um_least_rotation(u, p, lane & 1) : 0;
    const int rr = __shfl(r, lane | 1);
    if (!on || (lane & 1)) return;
    uint64_t h = 0;
    const UnitMotif m = unit_motif_from(u, p, r, rr, o.motif + uo, &h);
    o.strand[k] = (uint8_t)m.strand; o.rotation[k] = m.rotation; o.motif_len[k] = m.motif_len; o.hash[k] = (unsigned long long)h;
    o.read[k] = rd; o.bases[k] = rep_len; o.unit_off[k] = uo;
    o.copies[k] = m.motif_len > 0 ? (int64_t)nfu * (int64_t)(p / m.motif_len) : 0;
}

// exclusive offsets of the units' lengths, which the even lanes of the tile hold (every other lane passes 0); total = their sum
__device__ __forceinline__ int motif_tile_scan(int len, int lane, int &total)
{
    int incl = len;
    for (int d = 1; d < 2 * MOTIF_TILE; d <<= 1) { const int v = __shfl_up(incl, d); if (lane >= d) incl += v; }
    total = __shfl(incl, 2 * MOTIF_TILE - 1);
    return incl - len;
}

// strnlen(u, per) on a unit staged at a 4-byte boundary of LDS, four bytes a step (bytes behind per may be anything)
__device__ __forceinline__ int motif_strnlen(const uint8_t *u, int per)
{
    int p = 0;
    while (p < per) {
        const uint32_t w = *(const uint32_t *)(u + p);
        const uint32_t z = (w - 0x01010101u) & ~w & 0x80808080u;              // the lowest set bit marks the first zero byte
        if (z) { p += (__builtin_ctz(z) >> 3); break; }
        p += 4;
    }
    return p < per ? p : per;
}

__global__ void __launch_bounds__(64) mtr_k_unit_motif(RecordView v, ChainView ch, const int64_t *unit_base, int64_t total_repeats, int64_t total_unit_bytes, MotifRows o)
{
    __shared__ uint2 lds[MOTIF_TILE * MOTIF_SLOT_BYTES / 8];
    const int rd = blockIdx.x, lane = threadIdx.x;
    if (rd >= v.n_reads) return;
    if (rd == 0 && lane == 0) o.unit_off[total_repeats] = total_unit_bytes;
    const auto [idx, len, k0] = ch.read(rd);
    if (len <= 0) return;
    const DevRecord *src = v.read(rd).rec;
    int64_t ubase = unit_base[rd];
    for (int c = 0; c < len; c += MOTIF_TILE) {
        const int nt = len - c < MOTIF_TILE ? len - c : MOTIF_TILE;
        for (int q = lane; q < nt * (MOTIF_SLOT_BYTES / 8); q += 64) {         // word w of unit t; only the words the period covers
            const int t = q >> 6, w = q & 63;
            const DevRecord *r = src + idx[c + t];
            if (w * 8 < wire_period(r)) lds[q] = ((const uint2 *)r->unit)[w];
        }
        __syncthreads();
        const int t = lane >> 1;
        const bool on = t < nt;
        const uint8_t *u = (const uint8_t *)lds + (t & (MOTIF_TILE - 1)) * MOTIF_SLOT_BYTES;
        const DevRecord *r = src + idx[c + (on ? t : 0)];
        const int p = on ? motif_strnlen(u, wire_period(r)) : 0;               // strnlen(unit, rep_period), as chain_unit_len
        int total;
        const int before = motif_tile_scan(on && !(lane & 1) ? p : 0, lane, total);
        motif_row(u, p, on, lane, k0 + c + t, ubase + before, rd, r->f[4], r->f[2], o);
        ubase += total;
        __syncthreads();
    }
}

// mtr_test_unit_motifs: row k = units[unit_off[k] .. unit_off[k + 1]) of read read[k] with copies[k] and repeat_len[k]
__global__ void __launch_bounds__(64) mtr_k_unit_motif_rows(int32_t n, const uint8_t *units, const int64_t *unit_off, const int32_t *read, const int32_t *copies,
                                                             const int32_t *repeat_len, MotifRows o)
{
    __shared__ uint2 lds[MOTIF_TILE * MOTIF_SLOT_BYTES / 8];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * MOTIF_TILE;
    if (r0 >= n) return;
    if (r0 == 0 && lane == 0) o.unit_off[n] = unit_off[n];
    const int nt = n - r0 < MOTIF_TILE ? (int)(n - r0) : MOTIF_TILE;
    uint8_t *bytes = (uint8_t *)lds;
    for (int t = 0; t < nt; t++) {
        const int64_t uo = unit_off[r0 + t];
        const int p = (int)(unit_off[r0 + t + 1] - uo);
        for (int b = lane; b < p; b += 64) bytes[t * MOTIF_SLOT_BYTES + b] = units[uo + b];
    }
    __syncthreads();
    const int t = lane >> 1;
    const bool on = t < nt;
    const int64_t k = r0 + (on ? t : 0), uo = unit_off[k];
    motif_row(bytes + (t & (MOTIF_TILE - 1)) * MOTIF_SLOT_BYTES, (int)(unit_off[k + 1] - uo), on, lane, k, uo, read[k], copies[k], repeat_len[k], o);
}

// are the motifs of rows a and b equal as strings?
__device__ __forceinline__ bool motif_equal(const MotifRows &o, int64_t a, int64_t b)
{
    const int d = o.motif_len[a];
    if (d != o.motif_len[b] || o.hash[a] != o.hash[b]) return false;
    const uint8_t *ma = o.motif + o.unit_off[a], *mb = o.motif + o.unit_off[b];
    for (int t = 0; t < d; t += 8) {                       // eight bytes of each in flight, then one test
        unsigned diff = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) if (t + q < d) diff |= (unsigned)(ma[t + q] ^ mb[t + q]);
        if (diff) return false;
    }
    return true;
}

// slot_of[k] = the slot of k's motif.  The table has mask + 1 > n slots, all MOTIF_EMPTY before the launch: a probe meets an empty slot
// or its own motif after at most n others.
__global__ void __launch_bounds__(256) mtr_k_motif_insert(int32_t n, MotifRows o, unsigned *table, unsigned mask, unsigned *slot_of)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    unsigned s = um_start_slot(o.hash[k], mask);
    for (unsigned step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const unsigned old = atomicCAS(table + s, MOTIF_EMPTY, (unsigned)k);
        if (old == MOTIF_EMPTY) break;
        if (motif_equal(o, (int64_t)old, k)) { atomicMin(table + s, (unsigned)k); break; }
    }
    slot_of[k] = s;
}

// leader[k] = the first repeat of k's group; first[k] = 1 for such a repeat, lead_len[k] its motif's length (else 0, 0)
__global__ void __launch_bounds__(256) mtr_k_motif_leader(int32_t n, const int32_t *motif_len, const unsigned *table, const unsigned *slot_of,
                                                           int32_t *leader, int32_t *first, int32_t *lead_len)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int32_t l = (int32_t)table[slot_of[k]];
    leader[k] = l; first[k] = l == k ? 1 : 0; lead_len[k] = l == k ? motif_len[k] : 0;
}

// the columns of the catalogue per group (context-owned, zeroed before the launch where they are sums)
struct MotifGroups {
    int32_t *group;                                      // [n]
    int64_t *motif_off; uint8_t *motifs;                 // [G + 1], [M]
    int32_t *first, *repeats, *reads; int64_t *copies, *bases;     // [G]
};

__device__ __forceinline__ int64_t motif_wave_sum(int64_t x)
{
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// group_of = the exclusive sum of first[] (n + 1 entries, group_of[n] = G), len_off = that of lead_len[] (len_off[n] = M)
__global__ void __launch_bounds__(256) mtr_k_motif_groups(int32_t n, MotifRows o, const int32_t *leader, const int64_t *group_of, const int64_t *len_off, MotifGroups g)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = k < n;
    if (k == 0) g.motif_off[group_of[n]] = len_off[n];
    int32_t l = -1, gi = -1;
    bool new_read = false;
    if (in) {
        l = leader[k]; gi = (int32_t)group_of[l];
        g.group[k] = gi;
        if (l == k) {
            g.first[gi] = (int32_t)k; g.motif_off[gi] = len_off[k];
            const uint8_t *m = o.motif + o.unit_off[k];
            uint8_t *dst = g.motifs + len_off[k];
            const int d = o.motif_len[k];
            for (int t = 0; t < d; t += 8) {               // eight loads in flight, then eight stores
                uint8_t b[8];
#pragma unroll
                for (int q = 0; q < 8; q++) b[q] = t + q < d ? m[t + q] : (uint8_t)0;
#pragma unroll
                for (int q = 0; q < 8; q++) if (t + q < d) dst[t + q] = b[q];
            }
        }
        const int32_t rd = o.read[k];
        new_read = true;
        for (int64_t j = k - 1; j >= 0 && o.read[j] == rd; j--) if (leader[j] == l) { new_read = false; break; }
    }
    // the lanes of the wavefront that share a group add up first: its lowest lane makes the four atomics
    const int lane = threadIdx.x & 63;
    const int64_t cp = in ? o.copies[k] : 0, bs = in ? (int64_t)o.bases[k] : 0;
    unsigned long long todo = __ballot(in);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int32_t gl = __shfl(gi, lead);
        const bool mine = in && gi == gl;
        const unsigned long long mm = __ballot(mine), nr = __ballot(mine && new_read);
        const int64_t sc = motif_wave_sum(mine ? cp : 0), sb = motif_wave_sum(mine ? bs : 0);
        if (lane == lead) {
            atomicAdd(g.repeats + gl, (int32_t)__popcll(mm));
            if (nr) atomicAdd(g.reads + gl, (int32_t)__popcll(nr));
            atomicAdd((unsigned long long *)(g.copies + gl), (unsigned long long)sc);
            atomicAdd((unsigned long long *)(g.bases + gl), (unsigned long long)sb);
        }
        todo &= ~mm;
    }
}
