// catalog_build.hip.inc — a prepared locus catalogue built on the device (mtr_catalog_create): everything catalog_index, flank_slot_masks,
// motif_slots and partial_variants make on the host per call, made once from one uploaded copy of the loci's letters.  The host's pass over
// seq_off gives what lengths alone decide (the slots' lengths, the motifs' lengths and offsets); every kernel here reads bases.
//   mtr_k_catb_check     a lane per sequence whose length is legal: the first byte that is none of ACGT, as a key in the order of the text-taking
//                        calls' checks (all motifs, then the flanks locus by locus), minimised over the sequences.
//   mtr_k_catb_slots     a lane per slot (locus * 4 + j): the pattern's codes out of the ASCII into the lane's row of LDS (a byte array per
//                        lane in registers would be a stack), its eight masks (fbv_masks, flank_slot_masks' order), its K + 1 entries
//                        (si_seed_code at si_seed_offset, slot) at slot * (K + 1) + i: ascending (slot, i).
//   mtr_k_catb_count /   the stable LSD radix sort of the entries by code, 8 bits a pass (catalog_build.h): a workgroup of one wavefront per
//   mtr_k_catb_fill      tile of CB_TILE entries, 64 a step.  count: the tile's entries per digit, to hist[digit * tiles + tile], whose exclusive
//                        sums (mtr_k_scan_offsets) are where the tile's entries of a digit go.  fill: an entry lands at its digit's place
//                        plus its rank among the tile's entries of that digit - the steps before it (LDS) and its peers in lower lanes
//                        (ballots).  No atomic: the order is the input's, run after run.
//   mtr_k_catb_flags     per sorted entry: kept (it does not repeat its predecessor), head (its code differs from its predecessor's).
//   mtr_k_catb_compact   the kept entries' slots at their scanned places (the catalogue's `ent`); per head its code and the place of its first
//                        entry, at the head's scanned number - a run's count is the next head's place minus its own.
//   mtr_k_catb_table     a lane per distinct code: its filter bit by an atomic OR, its table slot claimed by a compare-and-swap of the run's
//                        count (0 -> count) along the probe sequence.  At most `cap` probes: a full table raises the status word.
//   mtr_k_catb_motifs    a lane per locus: the two single-strand units, their bits (mdp_motif_bits), and the four variants' bits.
#pragma once
#include "catalog.hip.inc"
#include "catalog_build.h"
#include "flank_bv.h"
#include "motif_dp.h"

#define CATB_ROW 68                     // bytes of LDS per lane in mtr_k_catb_slots: 64 codes, and 17 dwords spread the lanes over the banks
#define CATB_ERR_TABLE_FULL 16          // the status word of mtr_k_catb_table (beside DEV_ERR_INTERNAL)
#define CATB_NO_BAD_BYTE (~0ull)

struct CatbSrc { const char *seqs; const int64_t *off; int32_t n_loci; };      // sequence k of the loci: seqs[off[k] .. off[k + 1]), k = 3 * locus + which

// the check's key of byte t of a motif / of a flank (2 * locus + side); a length's refusal has t + 1 = 0 (the host makes those)
DEVINL unsigned long long catb_bad_key(int is_flank, long long index, int t) { return ((unsigned long long)is_flank << 62) | ((unsigned long long)index << 10) | (unsigned long long)(t + 1); }

__global__ __launch_bounds__(256) void mtr_k_catb_check(CatbSrc s, unsigned long long *bad)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= 3ll * s.n_loci) return;
    const int which = (int)(k % 3);
    const long long l = k / 3;
    const int64_t at = s.off[k], len = s.off[k + 1] - at;
    const bool legal = which == 1 ? len >= 1 && len < MTRC_MAX_PERIOD : len >= 1 && len <= FBV_MAX_M;
    if (!legal) return;
    for (int t = 0; t < (int)len; t++)
        if (cb_base_code(s.seqs[at + t]) < 0) {
            atomicMin(bad, which == 1 ? catb_bad_key(0, l, t) : catb_bad_key(1, 2 * l + (which == 2), t));
            return;
        }
}

struct CatbSlotArgs { CatbSrc s; const int32_t *plen; int32_t q, seeds; uint64_t *masks; uint32_t *keys; int32_t *vals; int32_t *status; };

__global__ __launch_bounds__(64) void mtr_k_catb_slots(CatbSlotArgs a)
{
    __shared__ uint8_t s_codes[64 * CATB_ROW];
    const int lane = lane_id();
    const long long slot = (long long)blockIdx.x * 64 + lane;
    if (slot >= 4ll * a.s.n_loci) return;
    const long long l = slot >> 2;
    const int j = (int)(slot & 3), m = a.plen[slot];
    const int64_t at = a.s.off[3 * l + 2 * (j & 1)];
    if (m < 1 || m > FBV_MAX_M || (int64_t)m != a.s.off[3 * l + 2 * (j & 1) + 1] - at || (long long)a.seeds * a.q > m) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); return; }
    uint8_t *p = s_codes + lane * CATB_ROW;
    cb_slot_codes(a.s.seqs + at, m, j, p);
    const FbvMasks<uint64_t> eq = fbv_masks<uint64_t>(p, m, 0), rev = fbv_masks<uint64_t>(p, m, 1);
    uint64_t *o = a.masks + slot * FL_MASKS;
    o[0] = eq.a; o[1] = eq.c; o[2] = eq.g; o[3] = eq.t; o[4] = rev.a; o[5] = rev.c; o[6] = rev.g; o[7] = rev.t;
    for (int i = 0; i < a.seeds; i++) {
        a.keys[slot * a.seeds + i] = si_seed_code(p + si_seed_offset(i, a.q), a.q);
        a.vals[slot * a.seeds + i] = (int32_t)slot;
    }
}

// a step of a tile: the lane's entry, and its peers among the step's 64
struct CatbStep { bool has; uint32_t key, digit; uint64_t peers; };
DEVINL CatbStep catb_step(const uint32_t *keys, long long e, long long n, int pass)
{
    CatbStep st;
    st.has = e < n;
    st.key = st.has ? keys[e] : 0u;
    st.digit = cb_digit(st.key, pass);
    uint64_t ballot[CB_DIGIT_BITS];
#pragma unroll
    for (int b = 0; b < CB_DIGIT_BITS; b++) ballot[b] = __ballot(st.has && ((st.digit >> b) & 1));
    st.peers = cb_peers(ballot, st.digit, __ballot(st.has));
    return st;
}

__global__ __launch_bounds__(64) void mtr_k_catb_count(const uint32_t *keys, long long n, int pass, int n_tiles, int32_t *hist)
{
    __shared__ uint32_t s_cnt[CB_DIGITS];
    const int lane = lane_id(), tile = (int)blockIdx.x;
    if (tile >= n_tiles) return;
    for (int d = lane; d < CB_DIGITS; d += 64) s_cnt[d] = 0;
    __syncthreads();
    for (int step = 0; step < CB_TILE / 64; step++) {
        const CatbStep st = catb_step(keys, (long long)tile * CB_TILE + step * 64 + lane, n, pass);
        if (st.has && cb_peer_last(st.peers, lane)) s_cnt[st.digit] += (uint32_t)__popcll(st.peers);
        __syncthreads();
    }
    for (int d = lane; d < CB_DIGITS; d += 64) hist[(size_t)d * (size_t)n_tiles + (size_t)tile] = (int32_t)s_cnt[d];
}

struct CatbFillArgs { const uint32_t *keys; const int32_t *vals; long long n; int32_t pass, n_tiles; const int64_t *first; uint32_t *keys_out; int32_t *vals_out; int32_t *status; };

__global__ __launch_bounds__(64) void mtr_k_catb_fill(CatbFillArgs a)
{
    __shared__ uint32_t s_at[CB_DIGITS];
    const int lane = lane_id(), tile = (int)blockIdx.x;
    if (tile >= a.n_tiles) return;
    for (int d = lane; d < CB_DIGITS; d += 64) s_at[d] = (uint32_t)a.first[(size_t)d * (size_t)a.n_tiles + (size_t)tile];
    __syncthreads();
    for (int step = 0; step < CB_TILE / 64; step++) {
        const long long e = (long long)tile * CB_TILE + step * 64 + lane;
        const CatbStep st = catb_step(a.keys, e, a.n, a.pass);
        const int32_t val = st.has ? a.vals[e] : 0;
        const long long pos = (long long)s_at[st.digit] + cb_peer_rank(st.peers, lane);
        __syncthreads();
        if (st.has && cb_peer_last(st.peers, lane)) s_at[st.digit] += (uint32_t)__popcll(st.peers);
        __syncthreads();
        if (st.has) {
            if (pos < a.n) { a.keys_out[pos] = st.key; a.vals_out[pos] = val; }
            else atomicCAS(a.status, 0, DEV_ERR_INTERNAL);
        }
    }
}

__global__ __launch_bounds__(256) void mtr_k_catb_flags(const uint32_t *keys, const int32_t *vals, long long n, int32_t *keep, int32_t *head)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const bool first = e == 0;
    const uint32_t key = keys[e], pk = first ? 0u : keys[e - 1];
    const int32_t slot = vals[e], ps = first ? 0 : vals[e - 1];
    keep[e] = cb_keep(first, key, slot, pk, ps) ? 1 : 0;
    head[e] = cb_head(first, key, pk) ? 1 : 0;
}

struct CatbCompactArgs {
    const uint32_t *keys; const int32_t *vals; long long n; const int32_t *keep, *head; const int64_t *keep_off, *head_off;
    long long E, distinct; int32_t *ent; uint32_t *rkey; int32_t *rfirst; int32_t *status;
};

__global__ __launch_bounds__(256) void mtr_k_catb_compact(CatbCompactArgs a)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    if (e == 0) a.rfirst[a.distinct] = (int32_t)a.E;
    if (!a.keep[e]) return;
    const long long k = a.keep_off[e];
    if (k < 0 || k >= a.E) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); return; }
    a.ent[k] = a.vals[e];
    if (!a.head[e]) return;
    const long long r = a.head_off[e];
    if (r < 0 || r >= a.distinct) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); return; }
    a.rkey[r] = a.keys[e]; a.rfirst[r] = (int32_t)k;
}

struct CatbTableArgs { const uint32_t *rkey; const int32_t *rfirst; long long distinct; uint32_t *filter; int32_t fbits; uint32_t *key; int32_t *run; uint32_t cap; int32_t *status; };

__global__ __launch_bounds__(256) void mtr_k_catb_table(CatbTableArgs a)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.distinct) return;
    const uint32_t code = a.rkey[r];
    const int32_t first = a.rfirst[r], count = a.rfirst[r + 1] - first;
    if (count < 1) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); return; }
    const uint32_t b = si_filter_bit(code, a.fbits);
    atomicOr(a.filter + (b >> 5), 1u << (b & 31));
    // (only heads come here: the codes are distinct, an occupied slot is another code's and no key is compared)
    for (uint32_t s = si_hash(code) & (a.cap - 1), n = 0; n < a.cap; s = (s + 1) & (a.cap - 1), n++)
        if (atomicCAS(a.run + 2 * (size_t)s + 1, 0, count) == 0) { a.key[s] = code; a.run[2 * (size_t)s] = first; return; }
    atomicCAS(a.status, 0, CATB_ERR_TABLE_FULL);
}

struct CatbMotifArgs { CatbSrc s; const int32_t *ulen, *unit_off; uint8_t *units; uint64_t *ubits, *vbits; int32_t *status; };

__global__ __launch_bounds__(256) void mtr_k_catb_motifs(CatbMotifArgs a)
{
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= a.s.n_loci) return;
    const int U = a.ulen[l];
    const int64_t at = a.s.off[3 * l + 1];
    const int32_t u0 = a.unit_off[2 * l], u1 = a.unit_off[2 * l + 1], u2 = a.unit_off[2 * l + 2];
    if (U < 1 || U >= MTRC_MAX_PERIOD || (int64_t)U != a.s.off[3 * l + 2] - at || u0 < 0 || u1 - u0 != U || u2 - u1 != U) { atomicCAS(a.status, 0, DEV_ERR_INTERNAL); return; }
    cb_motif_codes(a.s.seqs + at, U, 0, a.units + u0);
    cb_motif_codes(a.s.seqs + at, U, 1, a.units + u1);
    const uint64_t fwd = mdp_motif_bits(a.units + u0, U), rc = mdp_motif_bits(a.units + u1, U);
    a.ubits[2 * l] = fwd; a.ubits[2 * l + 1] = rc;
    const bool lanes = U <= MDP_MAX_U;                  // the partial call's variants: M, reversed M, rc M, reversed rc M (0 where it refuses the motif)
    a.vbits[4 * l] = lanes ? fwd : 0; a.vbits[4 * l + 1] = lanes ? cb_bits_reversed(fwd, U) : 0;
    a.vbits[4 * l + 2] = lanes ? rc : 0; a.vbits[4 * l + 3] = lanes ? cb_bits_reversed(rc, U) : 0;
}
