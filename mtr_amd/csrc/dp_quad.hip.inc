// dp_quad.hip.inc — FOUR two-parameter wrap-around DPs per wavefront, one per 16-lane DPP row, C columns per lane
// (reference wrap_around_DP.c:222-429: the forward passes of both parameter sets of wrap_around_DP, packed 16 + 16 bits as in
// dp_forward2p).
//
// Why: the kernels are bound by VALU issue (DESIGN.md 4.5), and a row of ONE alignment on 64 lanes pays ~28 instructions of
// per-row work (the 6-step segmented scan, the wrap through v_readlane, loop glue) for one or two column registers.  The staged
// chain has every alignment of the batch as a work item of its own, so alignments of DIFFERENT reads can share a wavefront:
// DP g lives in lanes 16 g .. 16 g + 15, lane l of it holds the C consecutive columns l C + 1 .. l C + C in C registers.  Inside a lane
// the deletion chain is a serial prefix maximum (two instructions per column, no cross-lane traffic); across the 16 lanes of a DP
// it is ONE four-step DPP scan (row_shr 1/2/4/8, never leaves the row) over the value that leaves each lane; the per-row work is
// shared by 4 x C column registers.  Recurrence, flags, best cell: exactly dp_forward2p's; DP g's matrix is its own contiguous piece of
// the block - row i at cells + g * DPQ_DP_BYTES + (i - 1) * 16 C, column j at byte j - 1 of it - so that the 16 lanes of a DP store
// one contiguous 16 C bytes per row and a traceback's window of 64 rows is 64 x 16 C contiguous bytes (with the four matrices
// interleaved row by row it was four times as many cache lines, and the tracebacks' window refills twice as slow);
// dp_traceback<., 1> reads DP g with codes = cells + g * DPQ_DP_BYTES, rstride = 16 C.
// A lane owns C bytes of the row but stores 4 (C <= 4) or 8: the bytes behind its own are the NEXT lane's first cells, fetched
// with one DPP move, so overlapping stores carry identical bytes (the row's last lane spills into the next row's first bytes,
// which that row's store rewrites; a matrix ends with 16 bytes of slack).  Scores are kept TIMES FOUR (gain, penalties and the D j offsets): every
// difference is then 0 or >= 4, so the three flags come out of v_pk_min_u16 with 1 / 2 / 4 already in place and one v_or3
// joins them; 16 bits then hold 4 (rows G + D (U + 2)) - see DPQ_FITS.
//
// The read windows differ per DP: a lane stages 16 bases of ITS DP's window, re-aligned so that the chunk's first base sits in bit
// 30 of lane 0's word; the word of the current 16 rows then comes from one ds_bpermute per 16 rows and the base from a uniform shift.
// A DP with fewer rows than the wavefront's longest keeps computing on "nothing matches" (its match table is cleared): H only
// decays, the best cell (strict '>') cannot move, and the rows it writes lie inside the quad's block.
#pragma once
#include "device_util.hip.inc"

struct DpQuad {
    const uint32_t *pk[4];      // packed read of each DP
    long long wlim[4];          // words readable from pk[g] (clamp for the window prefetch)
    int base[4], rows[4], U[4]; // rep[i] = org[base + i], i = 1 .. rows; unit length
    const uint8_t *unit[4];
    int n;                      // DPs present (1..4)
    int G[4], MM[4], D[4];      // dp_forward1p_g16 only: each DP's own parameter set
};
#define DPQ_SCALE 4
// unsigned 16-bit arithmetic on scores times SC (dp_forward2p's bound is DP2P_MAX_ROWS for scores times one)
#define DPQ_FITS_SC(SC, rows, U, G, D) ((long)(SC) * ((long)(rows) * (long)(G) + (long)(D) * ((long)(U) + 2)) < 65000L)
#define DPQ_FITS(rows, U, G, D) DPQ_FITS_SC(DPQ_SCALE, rows, U, G, D)
#define DPQ_COLS(U) (((U) + 15) >> 4)                       /* columns per lane of a 16-lane DP for a unit of U bases (1 .. 8) */
#define DPQ_COLS64(U) (((U) + 63) >> 6)                     /* columns per lane of a DP on the whole wavefront (GL = 64) */
#define DPQ_ROW_BYTES_G(GL, C) ((GL) * (C))                  /* bytes of one row of one DP (row stride of its matrix) */
#define DPQ_DP_BYTES_G(GL, C, maxrows) ((size_t)(maxrows) * DPQ_ROW_BYTES_G(GL, C) + 16)   /* one DP's matrix + the slack its last row's store spills into */
#define DPQ_ROW_BYTES(C) DPQ_ROW_BYTES_G(16, C)
#define DPQ_DP_BYTES(C, maxrows) DPQ_DP_BYTES_G(16, C, maxrows)
#define DPQ_BLOCK_BYTES(C, maxrows) (4 * DPQ_DP_BYTES(C, maxrows))
/* dp_forward1p_g16<., 16, ., true>: TWO rows per byte row (row 2r+1 in the low nibble, row 2r+2 in the high one) */
#define DPQP_DP_BYTES_G(GL, C, maxrows) ((size_t)(((maxrows) + 1) >> 1) * DPQ_ROW_BYTES_G(GL, C) + 16)
#define DPQP_DP_BYTES(C, maxrows) DPQP_DP_BYTES_G(16, C, maxrows)
#define DPQP_BLOCK_BYTES(C, maxrows) (4 * DPQP_DP_BYTES(C, maxrows))

// GL = lanes per DP: 16 (four DPs per wavefront) or 64 (ONE DP on the whole wavefront, C columns per lane: units of 129..256 bases,
// which the chunked dp_forward2p<4> takes at ~250 instructions a row).  SC = what the scores are multiplied by: 4 (see above) or 1
// (windows beyond DPQ_FITS: the flags then take two shifts more per column).
//
// GL = 8 (units of up to 32 bases, C <= 4): EIGHT DPs per wavefront, two per DPP row - a unit of at most 16 bases has one column per lane of a 16-lane DP
// and pays a quarter of the per-row work whatever its length.  The members come as DpLanes, every lane holding the values of ITS DP (no selects over
// eight members), and the best cells go back the same way.  What differs in the row loop: a DP's first lane starts a scan segment of its own (a constant
// lane mask joins the match lanes: the row's scan then carries nothing over from the DP before it), and it takes no incoming value and the wrap as its
// diagonal, which the row's first lane gets from the DPP move itself; the scan has three steps.
struct DpLanes {                // per lane: the DP of lanes 8 d .. 8 d + 7 (member d of the pass); rows = 0 and U = 0: no such member
    const uint32_t *pk; long long wlim; int base, rows, U; const uint8_t *unit;
};
#define DPO_BLOCK_BYTES(C, maxrows) (8 * DPQ_DP_BYTES_G(8, C, maxrows))
DEVINL void scan_max_u32_x2_row8(unsigned &a, unsigned &b)
{   // scan_max_u32_x2_row16 without its last step: for keys that grow from one half of the row to the other
    unsigned s, t;
#define MTR_SCAN_STEP(ctrl) \
    s = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a, ctrl, 0xf, 0xf, false); \
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b, ctrl, 0xf, 0xf, false); \
    a = s > a ? s : a; b = t > b ? t : b;
    MTR_SCAN_STEP(0x111) MTR_SCAN_STEP(0x112) MTR_SCAN_STEP(0x114)
#undef MTR_SCAN_STEP
}
template <int C, int GL = 16, int SC = DPQ_SCALE, class Q = DpQuad, class B = int[4][2][3]>
DEVINL void dp_forward2p_g16(const Q &q, int G0, int MM0, int D0, int G1, int MM1, int D1, uint8_t *cells, int maxrows, B &best)
{
    static_assert(C >= 1 && C <= 8 && (GL == 16 || GL == 64 || (GL == 8 && C <= 4 && SC == 4)) && (SC == 1 || SC == 4), "columns per lane, lanes per DP, score scale");
    constexpr int NG = 64 / GL;
    int lane = lane_id();
    // (GL = 8: what a pass derives from the lane alone - its first cell's address, D l C, the crossbar addresses, for each C - is not to be formed at the top of
    //  the calling kernel for all widths and kept there in registers that the kernel's widest passes then spill)
    if (GL == 8) asm volatile("" : "+v"(lane));
    const int g = lane / GL, l = lane % GL;
    unsigned Gpk = SC * ((unsigned)G0 | ((unsigned)G1 << 16)), MMpk = SC * ((unsigned)MM0 | ((unsigned)MM1 << 16)), Dpk = SC * ((unsigned)D0 | ((unsigned)D1 << 16));
    unsigned ONE = 0x00010001u, TWO = 0x00020002u, FOUR = 0x00040004u, SEL_HI = 0x07060100u, C8 = 0x00080008u;
    asm volatile("" : "+v"(ONE), "+v"(TWO), "+v"(FOUR), "+v"(SEL_HI), "+v"(C8));
    unsigned SEL_K0 = 0x0c040100u, SEL_K1 = 0x0c040302u, SEL_S = 0x05040100u, SEL_LO = 0x05040100u, SEL_P1 = 0x07060302u, K4N = ~0x00040004u;
    asm volatile("" : "+s"(MMpk), "+s"(Dpk), "+s"(SEL_K0), "+s"(SEL_K1), "+s"(SEL_S), "+s"(SEL_LO), "+s"(SEL_P1), "+s"(K4N));
    // ---- this lane's DP
    int Ul, basel, rowsl; const uint8_t *up_; const uint32_t *pkl; long long wl;
    if constexpr (GL == 8) {
        Ul = q.U; basel = q.base; rowsl = q.rows; up_ = q.unit; pkl = q.pk; wl = q.wlim;
        if (rowsl <= 0) { Ul = 0; rowsl = 0; }
    } else {
        Ul = q.U[0]; basel = q.base[0]; rowsl = q.rows[0]; up_ = q.unit[0]; pkl = q.pk[0]; wl = q.wlim[0];
        if (g == 1) { Ul = q.U[1]; basel = q.base[1]; rowsl = q.rows[1]; up_ = q.unit[1]; pkl = q.pk[1]; wl = q.wlim[1]; }
        if (g == 2) { Ul = q.U[2]; basel = q.base[2]; rowsl = q.rows[2]; up_ = q.unit[2]; pkl = q.pk[2]; wl = q.wlim[2]; }
        if (g == 3) { Ul = q.U[3]; basel = q.base[3]; rowsl = q.rows[3]; up_ = q.unit[3]; pkl = q.pk[3]; wl = q.wlim[3]; }
        if (g >= q.n) { Ul = 0; rowsl = 0; }
    }
    // the unit's base of each of the lane's columns, one byte each (4 = no such column: no read base equals it).  A column's match is
    // ONE compare of its byte with the row's base (the byte picked by the instruction itself, SDWA), whose result is a scalar mask: "no
    // match so far in this lane" is then scalar arithmetic on masks.  (Before: a table of match bits per base, one v_perm per row and
    // an AND + compare per column and per prefix: three vector instructions per column more.)
    unsigned ubw[2] = { 0x04040404u, 0x04040404u };
    // The chain runs on g = H + D j (a step to the right then costs nothing: a prefix maximum).  Inside a lane j counts from the lane's own
    // first column: the per-column constants D (c + 1) and D (c + 1) + G are then the same for every lane (literals / scalars: no register,
    // where 2 C lane constants did not fit and the compiler formed them again in every row, ~6 instructions per column); the lane's offset
    // D l C is added to what leaves the lane before the scan over the lanes and taken off what comes in (Dlane)
    unsigned Kc[C], KGc[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int j = l * C + c + 1;
        if (j <= Ul) ubw[c >> 2] = (ubw[c >> 2] & ~(0xffu << (8 * (c & 3)))) | ((unsigned)(up_[j - 1] & 3) << (8 * (c & 3)));
        Kc[c] = SC * ((unsigned)(D0 * (c + 1)) | ((unsigned)(D1 * (c + 1)) << 16));
        KGc[c] = Kc[c] + Gpk;
    }
    const unsigned Dlane = SC * ((unsigned)(D0 * l * C) | ((unsigned)(D1 * l * C) << 16));
    {
        int landed = lane_val((int)(ubw[0] ^ ubw[1]), 0);
        asm volatile("" :: "s"(landed));
    }
    // column U of this lane's DP: lane lU of the row, register rU
    const int lU = Ul > 0 ? (Ul - 1) / C : 0, rU = Ul > 0 ? (Ul - 1) % C : 0;
    const int hu_addr = (g * GL + lU) << 2;
    const int lUs = GL == 64 ? uni(lU) : 0;                     // (GL = 64: one DP, every lane agrees on lU)
    bool is_r[C];
#pragma unroll
    for (int c = 0; c < C; c++) is_r[c] = rU == c;
    const bool lane0 = l == 0;
    const int grp_addr = (g * GL) << 2;                         // ds_bpermute address of the DP's first lane
    // best cell per column PAIR (SC = 4: a v_max3 takes two columns' keys, and half the registers): key = H << 16 | (0x7FFF - i) << 1 | first column
    // of the pair - largest H, then smallest i, then smallest j, as the per-column keys H << 16 | 0xFFFF - i of SC = 1 (rows beyond 32767 there)
    // Two invariants the pair keys rest on (ADVICE r4):
    //  (1) the row index has 15 bits.  BKP is SC == 4 only, and a DP takes the SC = 4 pass only under DPQ_FITS: 4 (rows G + D (U + 2)) < 65000 with
    //      G >= 1, i.e. rows < 16250 (static_assert below);
    //  (2) the column test `j <= Ul` runs on the pair's WINNER only.  A column beyond the unit (its byte is 4: it never matches) holds
    //      max(0, diag - MM, up - D, left - D) of cells that are, by induction over the rows, below the best value of the unit's last column by at
    //      least min(MM, D) >= 1 (every parameter set of the reference has MM, D >= 1: (1,1,3), (1,3,1), (5,1,1); nothing saturates under DPQ_FITS) -
    //      so such a column never wins a pair whose other column is real, and a pair of two such columns is dropped by the test.
    constexpr bool BKP = SC == 4;
    static_assert(65000 / DPQ_SCALE <= 0x7FFF, "DPQ_FITS must keep the rows of an SC = 4 pass within the 15 bits of the pair keys");
    constexpr int NBK = BKP ? (C + 1) / 2 : C;
    unsigned P[C], bk0[NBK], bk1[NBK];
#pragma unroll
    for (int c = 0; c < C; c++) P[c] = 0u;
#pragma unroll
    for (int c = 0; c < NBK; c++) { bk0[c] = 0u; bk1[c] = 0u; }
    unsigned wrapv = 0u;                                        // H(i-1, U) of this lane's DP (all lanes of the row hold it)
    // rows after which a DP is over: the next such row is a scalar, the test per row a scalar compare
    int next_done = maxrows + 1;
    if constexpr (GL == 8) next_done = uni(-wave_max_i32(-rowsl));
    else {
#pragma unroll
        for (int h = 0; h < NG; h++) { const int r = h < q.n ? q.rows[h] : 0; if (r < next_done) next_done = r; }
    }
    const unsigned long long seg_heads = GL == 8 ? 0x0101010101010101ull : 0ull;     // GL = 8: every DP's first lane starts a scan segment
    if (rowsl <= 0) { ubw[0] = 0x04040404u; ubw[1] = 0x04040404u; }
    uint8_t *crow = cells + (size_t)g * DPQ_DP_BYTES_G(GL, C, maxrows) + (size_t)l * C;
    int i = 1;
    constexpr int CHUNK = 16 * GL - 16;                         // rows per staged window chunk: that many bases starting anywhere in a word span at most GL words
    for (int t0 = 0; t0 < maxrows; t0 += CHUNK) {
        // ---- stage the chunk's window: lane l holds the 16 bases pos0 + 16 l .. of ITS DP, first base in bit 30
        const int pos0 = basel + 1 + t0;
        long long w0 = (long long)(pos0 >> 4) + l;
        long long w1 = w0 + 1;
        if (w0 > wl - 1) w0 = wl - 1;
        if (w1 > wl - 1) w1 = wl - 1;
        if (w0 < 0) w0 = 0;
        if (w1 < 0) w1 = 0;
        const uint32_t wa = pkl[w0], wb = pkl[w1];
        const unsigned sh = 2u * (unsigned)(pos0 & 15);
        const uint32_t A = (uint32_t)(((((unsigned long long)wa) << 32) | (unsigned long long)wb) >> (32u - sh));
        {
            int landed = lane_val((int)A, 0);
            asm volatile("" :: "s"(landed));
        }
        const int i_chunk_end = t0 + CHUNK < maxrows ? t0 + CHUNK : maxrows;
        for (int wd = 0; i <= i_chunk_end; wd++) {
            const uint32_t wcur = (uint32_t)__builtin_amdgcn_ds_bpermute(grp_addr + (wd << 2), (int)A);
            const int i_w_end = i + 15 < i_chunk_end ? i + 15 : i_chunk_end;
            int bsh = 30;
#pragma unroll 1
            for (; i <= i_w_end; i++, bsh -= 2) {
                if (i > next_done) {                            // rare: some DP of the wavefront has had its last row
                    if (i > rowsl) { ubw[0] = 0x04040404u; ubw[1] = 0x04040404u; }
                    next_done = maxrows + 1;
                    if constexpr (GL == 8) next_done = uni(-wave_max_i32(-(rowsl >= i ? rowsl : maxrows + 1)));
                    else {
#pragma unroll
                        for (int h = 0; h < NG; h++) { const int r = h < q.n ? q.rows[h] : 0; if (r >= i && r < next_done) next_done = r; }
                    }
                }
                const unsigned xi = __builtin_amdgcn_ubfe(wcur, (unsigned)bsh, 2u);
                const unsigned inv_i = 0xFFFFu - (unsigned)i;
                // ---- phase A: the lane's own chain, as if nothing came in from the left
                unsigned s[C], t1s[C];
                bool mt[C], nh[C];
                unsigned sprev = 0u;
                bool nhp = true;
                unsigned diag0 = GL != 64 ? (unsigned)row_shift_up1((int)P[C - 1], (int)wrapv) : (unsigned)shift_up1((int)P[C - 1], (int)wrapv);
                if (GL == 8) diag0 = lane0 ? wrapv : diag0;                         // (the DP in the row's second half: its first lane is no row's first)
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const unsigned diag = c == 0 ? diag0 : P[c - 1];
                    const unsigned upv = P[c];
                    const bool m = ((ubw[c >> 2] >> (8 * (c & 3))) & 0xffu) == xi;
                    const unsigned t1 = pk_sub_sat(diag, MMpk), t2 = pk_sub_sat(upv, Dpk);
                    const unsigned gnm = pk_max(t1, t2) + Kc[c];                    // no carry between the halves: plain adds
                    const unsigned gm = diag + KGc[c];
                    const unsigned ch = pk_max(gnm, sprev);
                    const unsigned sc = m ? gm : ch;
                    s[c] = sc; t1s[c] = t1; mt[c] = m;
                    nhp = nhp && !m; nh[c] = nhp;
                    sprev = sc;
                }
                // ---- what arrives from the left: segmented prefix maximum over the row's 16 lanes of the value leaving each lane
                const unsigned long long hm = __ballot(!nhp) | seg_heads;
                const unsigned seg = (unsigned)mbcnt(hm >> 1);
                const unsigned sout = sprev + Dlane;                                // what leaves the lane, counted from column 1 of the DP
                unsigned k0 = __builtin_amdgcn_perm(seg, sout, SEL_K0);
                unsigned k1 = __builtin_amdgcn_perm(seg, sout, SEL_K1);
                if (GL == 8) scan_max_u32_x2_row8(k0, k1); else if (GL == 16) scan_max_u32_x2_row16(k0, k1); else scan_max_u32_x2(k0, k1);
                const unsigned S = __builtin_amdgcn_perm(k1, k0, SEL_S);
                // the DP's first lane (column 1): nothing comes in.  Every other lane: at least what left the lane before it, which is at least
                // D l C in both halves (g >= D j) - the subtraction borrows nothing
                unsigned e = (GL != 64 ? (unsigned)row_shift_up1((int)S, 0) : (unsigned)shift_up1((int)S, 0)) - Dlane;
                if (GL == 8) e = lane0 ? 0u : e;
                // ---- phase B: the incoming value reaches the columns before the lane's first match
                unsigned f[8];
#pragma unroll
                for (int c = C; c < 8; c++) f[c] = 0u;
                unsigned hgp = e;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const unsigned mx = pk_max(s[c], e);
                    const unsigned hg = nh[c] ? mx : s[c];
                    const unsigned H = hg - Kc[c];
                    const unsigned nz = pk_nonzero(H, ONE);                          // scores are multiples of four (SC = 4):
                    const unsigned nx = pk_nonzero(H - t1s[c], SC == 4 ? TWO : ONE); //   H >= t1 in every half of a non-match cell; 0 or 2
                    const unsigned nd = pk_nonzero(hg - hgp, SC == 4 ? FOUR : ONE);  //   hg >= hgp likewise: deletion <=> equal; 0 or 4
                    unsigned fl;
                    if (SC == 4) asm("v_or3_b32 %0, %1, %2, %3" : "=v"(fl) : "v"(nz), "v"(nx), "v"(nd));
                    else fl = lshl_or<1>(nx, lshl_or<2>(nd, nz));
                    fl = mt[c] ? C8 : fl;
                    f[c] = fl;
                    if (!BKP) {
                        const unsigned q0 = (H << 16) | inv_i, q1 = __builtin_amdgcn_perm(H, inv_i, SEL_HI);
                        bk0[c] = q0 > bk0[c] ? q0 : bk0[c];
                        bk1[c] = q1 > bk1[c] ? q1 : bk1[c];
                    }
                    P[c] = H;
                    hgp = hg;
                }
                if (BKP) {
                    const unsigned r0 = (0x7FFFu - (unsigned)i) << 1, r1 = r0 | 1u;
#pragma unroll
                    for (int c = 0; c + 1 < C; c += 2) {
                        const unsigned a0 = (P[c] << 16) | r1, b0 = (P[c + 1] << 16) | r0;
                        const unsigned a1 = __builtin_amdgcn_perm(P[c], r1, SEL_HI), b1 = __builtin_amdgcn_perm(P[c + 1], r0, SEL_HI);
                        bk0[c >> 1] = max3_u32(bk0[c >> 1], a0, b0);
                        bk1[c >> 1] = max3_u32(bk1[c >> 1], a1, b1);
                    }
                    if (C & 1) {
                        const unsigned a0 = (P[C - 1] << 16) | r1, a1 = __builtin_amdgcn_perm(P[C - 1], r1, SEL_HI);
                        bk0[C >> 1] = a0 > bk0[C >> 1] ? a0 : bk0[C >> 1];
                        bk1[C >> 1] = a1 > bk1[C >> 1] ? a1 : bk1[C >> 1];
                    }
                }
                // ---- H(i,U): next row's wrap, and column 1's "left" in the traceback's deletion test (:302/:314)
                unsigned hsel = P[0];
#pragma unroll
                for (int c = 1; c < C; c++) hsel = is_r[c] ? P[c] : hsel;
                // (one DP on the whole wavefront: the lane that holds column U is the same for every lane - a v_readlane instead of the LDS crossbar's
                //  round trip, which sits on the row's critical path: H(i, U) is the next row's first diagonal)
                wrapv = GL == 64 ? (unsigned)__builtin_amdgcn_readlane((int)hsel, lUs) : (unsigned)__builtin_amdgcn_ds_bpermute(hu_addr, (int)hsel);
                {
                    unsigned nd0 = pk_nonzero(pk_sub(pk_add(P[0], Dpk), wrapv), SC == 4 ? FOUR : ONE);
                    if (SC != 4) nd0 <<= 2;
                    unsigned f0;
                    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(f0) : "v"(f[0]), "s"(K4N), "v"(nd0));
                    f[0] = (lane0 && !mt[0]) ? f0 : f[0];
                }
                // ---- cells: byte c = flags of set 0 | flags of set 1 << 4; bytes behind the lane's own C = the next lane's first cells
                const unsigned F01 = lshl_or<8>(f[1], f[0]), F23 = lshl_or<8>(f[3], f[2]);
                unsigned lo = lshl_or<4>(__builtin_amdgcn_perm(F23, F01, SEL_P1), __builtin_amdgcn_perm(F23, F01, SEL_LO));
                if (C > 4) {
                    const unsigned F45 = C > 5 ? lshl_or<8>(f[5], f[4]) : f[4], F67 = C > 7 ? lshl_or<8>(f[7], f[6]) : f[6];
                    unsigned hi = lshl_or<4>(__builtin_amdgcn_perm(F67, F45, SEL_P1), __builtin_amdgcn_perm(F67, F45, SEL_LO));
                    if (C < 8) {
                        const unsigned nlo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x130, 0xf, 0xf, false);   // wave_shl:1: the next lane's first four cells
                        hi = lshl_or<8 * (C > 4 && C < 8 ? C - 4 : 0)>(nlo, hi);
                    }
                    *(uint2 *)crow = make_uint2(lo, hi);
                } else if (C == 1) {
                    *crow = (uint8_t)lo;
                } else {
                    if (C < 4) {
                        const unsigned nlo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x130, 0xf, 0xf, false);
                        lo = lshl_or<8 * (C < 4 ? C : 0)>(nlo, lo);
                    }
                    *(uint32_t *)crow = lo;
                }
                crow += DPQ_ROW_BYTES_G(GL, C);
                loop_join();
            }
            loop_join();
        }
        loop_join();
    }
    // ---- best cell per DP and parameter set: largest value, then smallest i, then smallest j
#pragma unroll
    for (int d = 0; d < 2; d++) {
        int v = 0, vi = 0, vj = 0;
#pragma unroll
        for (int t = 0; t < NBK; t++) {
            const unsigned bk = d == 0 ? bk0[t] : bk1[t];
            const int c = BKP ? 2 * t + 1 - (int)(bk & 1u) : t;
            const int j = l * C + c + 1;
            const int bvc = (int)(bk >> 16), bic = BKP ? (int)(0x7FFFu - ((bk & 0xFFFFu) >> 1)) : (int)(0xFFFFu - (bk & 0xFFFFu));
            if (j <= Ul && (bvc > v || (bvc == v && bvc > 0 && bic < vi))) { v = bvc; vi = bic; vj = j; }
        }
        for (int dd = GL / 2; dd > 0; dd >>= 1) {
            const int ov = __shfl_xor(v, dd, 64), oi = __shfl_xor(vi, dd, 64), oj = __shfl_xor(vj, dd, 64);
            const bool take = (ov > v) || (ov == v && ov > 0 && (oi < vi || (oi == vi && oj < vj)));
            if (take) { v = ov; vi = oi; vj = oj; }
        }
        if constexpr (GL == 8) { best[d][0] = v / SC; best[d][1] = vi; best[d][2] = vj; }       // (every lane of a DP holds its DP's)
        else {
#pragma unroll
            for (int h = 0; h < NG; h++) { best[h][d][0] = lane_val(v, GL * h) / SC; best[h][d][1] = lane_val(vi, GL * h); best[h][d][2] = lane_val(vj, GL * h); }
        }
    }
}


// ---- ONE parameter set per DP (revise_representative_unit_sub's vote DP and the re-alignment behind it, consensus.c:851-962,
// :1067/:1076): the same layout, four DPs per wavefront (each with its OWN scores: a pass may mix the rounds of different revisions), C columns per
// lane, 16-bit scores times four in 32-bit registers.  The
// recurrence runs on the 16-bit VOP2 instructions (v_max_u16 / v_min_u16 / v_sub_u16 clamp) and plain 32-bit adds, which this chip
// issues at twice the rate of packed, DPP and VOP3-only ones (profiles/r03_issue_costs.txt).  Cells: four flags per cell.  PAIR = false: one
// byte per cell, the flags in the low nibble - dp_traceback<., 1> with psel = 0.  PAIR = true (round 4: the revisions' passes wrote 22.7 GB per
// 10 000-read launch, half of every byte empty): a byte holds the cells of TWO rows - the odd row's packed bytes wait in two registers, the even row's
// join them shifted by four, and ONE store (and one neighbour exchange) serves both rows: half the bytes, half the stores, two instructions more per
// row pair; a DP's matrix is ceil(rows / 2) byte rows (DPQP_DP_BYTES), read by dp_traceback<., 3>.
DEVINL unsigned u16_max(unsigned a, unsigned b) { unsigned r; asm("v_max_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
DEVINL unsigned u16_min(unsigned a, unsigned b) { unsigned r; asm("v_min_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
DEVINL unsigned u16_sub_sat(unsigned a, unsigned b) { unsigned r; asm("v_sub_u16_e64 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b)); return r; }
DEVINL unsigned u16_sub(unsigned a, unsigned b) { unsigned r; asm("v_sub_u16_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
DEVINL unsigned scan_max_u32_row16(unsigned a)
{
    unsigned s;
#define MTR_SCAN_STEP(ctrl) s = (unsigned)__builtin_amdgcn_update_dpp(0, (int)a, ctrl, 0xf, 0xf, false); a = s > a ? s : a;
    MTR_SCAN_STEP(0x111) MTR_SCAN_STEP(0x112) MTR_SCAN_STEP(0x114) MTR_SCAN_STEP(0x118)
#undef MTR_SCAN_STEP
    return a;
}
template <int C, int GL = 16, int SC = DPQ_SCALE, bool PAIR = false>
DEVINL void dp_forward1p_g16(const DpQuad &q, uint8_t *cells, int maxrows, int (&best)[4][3])
{
    static_assert(C >= 1 && C <= 8 && (GL == 16 || GL == 64) && (SC == 1 || SC == 4), "columns per lane, lanes per DP, score scale");
    constexpr int NG = 64 / GL;
    const int lane = lane_id();
    const int g = lane / GL, l = lane % GL;
    unsigned ONE = 1u, TWO = 2u, FOUR = 4u, EIGHT = 8u;
    asm volatile("" : "+v"(ONE), "+v"(TWO), "+v"(FOUR), "+v"(EIGHT));
    int Ul = q.U[0], basel = q.base[0], rowsl = q.rows[0]; const uint8_t *up_ = q.unit[0]; const uint32_t *pkl = q.pk[0]; long long wl = q.wlim[0];
    int Gl = q.G[0], MMl = q.MM[0], Dl = q.D[0];
    if (g == 1) { Ul = q.U[1]; basel = q.base[1]; rowsl = q.rows[1]; up_ = q.unit[1]; pkl = q.pk[1]; wl = q.wlim[1]; Gl = q.G[1]; MMl = q.MM[1]; Dl = q.D[1]; }
    if (g == 2) { Ul = q.U[2]; basel = q.base[2]; rowsl = q.rows[2]; up_ = q.unit[2]; pkl = q.pk[2]; wl = q.wlim[2]; Gl = q.G[2]; MMl = q.MM[2]; Dl = q.D[2]; }
    if (g == 3) { Ul = q.U[3]; basel = q.base[3]; rowsl = q.rows[3]; up_ = q.unit[3]; pkl = q.pk[3]; wl = q.wlim[3]; Gl = q.G[3]; MMl = q.MM[3]; Dl = q.D[3]; }
    if (g >= q.n) { Ul = 0; rowsl = 0; }
    const unsigned Gs = SC * (unsigned)Gl, MMs = SC * (unsigned)MMl, Ds = SC * (unsigned)Dl;      // per lane: the DPs of a pass need not share their scores
    // the unit's base of each of the lane's columns, one byte each (4 = no such column: no read base equals it).  A column's match is
    // ONE compare of its byte with the row's base, whose result is a scalar mask: "no match so far in this lane" is then scalar arithmetic
    unsigned ubw[2] = { 0x04040404u, 0x04040404u };
    unsigned Dj[C], GDj[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int j = l * C + c + 1;
        if (j <= Ul) ubw[c >> 2] = (ubw[c >> 2] & ~(0xffu << (8 * (c & 3)))) | ((unsigned)(up_[j - 1] & 3) << (8 * (c & 3)));
        Dj[c] = Ds * (unsigned)j;
        GDj[c] = Dj[c] + Gs;
    }
    {
        int landed = lane_val((int)(ubw[0] ^ ubw[1]), 0);
        asm volatile("" :: "s"(landed));
    }
    const int lU = Ul > 0 ? (Ul - 1) / C : 0, rU = Ul > 0 ? (Ul - 1) % C : 0;
    const int hu_addr = (g * GL + lU) << 2;
    const int lUs = GL == 64 ? uni(lU) : 0;                     // (GL = 64: one DP, every lane agrees on lU)
    bool is_r[C];
#pragma unroll
    for (int c = 0; c < C; c++) is_r[c] = rU == c;
    const bool lane0 = l == 0;
    const int grp_addr = (g * GL) << 2;
    constexpr bool BKP = SC == 4;                               // best cell per column pair, as dp_forward2p_g16
    constexpr int NBK = BKP ? (C + 1) / 2 : C;
    unsigned P[C], bk[NBK];
#pragma unroll
    for (int c = 0; c < C; c++) P[c] = 0u;
#pragma unroll
    for (int c = 0; c < NBK; c++) bk[c] = 0u;
    unsigned wrapv = 0u;
    int next_done = maxrows + 1;
#pragma unroll
    for (int h = 0; h < NG; h++) { const int r = h < q.n ? q.rows[h] : 0; if (r < next_done) next_done = r; }
    if (rowsl <= 0) { ubw[0] = 0x04040404u; ubw[1] = 0x04040404u; }
    uint8_t *crow = cells + (size_t)g * (PAIR ? DPQP_DP_BYTES_G(GL, C, maxrows) : DPQ_DP_BYTES_G(GL, C, maxrows)) + (size_t)l * C;
    unsigned loP = 0u, hiP = 0u;                                // PAIR: the odd row's packed cells, waiting for the even row
    // the row's packed cells (byte c = the lane's c-th cell) to memory: the bytes behind the lane's own C are the NEXT lane's first cells
    auto store_cells = [&](unsigned lo, unsigned hi) {
        if (C > 4) {
            if (C < 8) {
                const unsigned nlo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x130, 0xf, 0xf, false);
                hi |= nlo << (8 * (C > 4 && C < 8 ? C - 4 : 0));
            }
            *(uint2 *)crow = make_uint2(lo, hi);
        } else if (C == 1) {
            *crow = (uint8_t)lo;
        } else {
            if (C < 4) {
                const unsigned nlo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x130, 0xf, 0xf, false);
                lo |= nlo << (8 * (C < 4 ? C : 0));
            }
            *(uint32_t *)crow = lo;
        }
        crow += DPQ_ROW_BYTES_G(GL, C);
    };
    int i = 1;
    constexpr int CHUNK = 16 * GL - 16;                         // rows per staged window chunk: that many bases starting anywhere in a word span at most GL words (even: a chunk starts on an odd row)
    for (int t0 = 0; t0 < maxrows; t0 += CHUNK) {
        const int pos0 = basel + 1 + t0;
        long long w0 = (long long)(pos0 >> 4) + l;
        long long w1 = w0 + 1;
        if (w0 > wl - 1) w0 = wl - 1;
        if (w1 > wl - 1) w1 = wl - 1;
        if (w0 < 0) w0 = 0;
        if (w1 < 0) w1 = 0;
        const uint32_t wa = pkl[w0], wb = pkl[w1];
        const unsigned sh = 2u * (unsigned)(pos0 & 15);
        const uint32_t A = (uint32_t)(((((unsigned long long)wa) << 32) | (unsigned long long)wb) >> (32u - sh));
        {
            int landed = lane_val((int)A, 0);
            asm volatile("" :: "s"(landed));
        }
        const int i_chunk_end = t0 + CHUNK < maxrows ? t0 + CHUNK : maxrows;
        for (int wd = 0; i <= i_chunk_end; wd++) {
            const uint32_t wcur = (uint32_t)__builtin_amdgcn_ds_bpermute(grp_addr + (wd << 2), (int)A);
            const int i_w_end = i + 15 < i_chunk_end ? i + 15 : i_chunk_end;
            int bsh = 30;
#pragma unroll 1
            for (; i <= i_w_end; i++, bsh -= 2) {
                if (i > next_done) {
                    if (i > rowsl) { ubw[0] = 0x04040404u; ubw[1] = 0x04040404u; }
                    next_done = maxrows + 1;
#pragma unroll
                    for (int h = 0; h < NG; h++) { const int r = h < q.n ? q.rows[h] : 0; if (r >= i && r < next_done) next_done = r; }
                }
                const unsigned xi = __builtin_amdgcn_ubfe(wcur, (unsigned)bsh, 2u);
                const unsigned inv_i = 0xFFFFu - (unsigned)i;
                unsigned s[C], t1s[C];
                bool mt[C], nh[C];
                unsigned sprev = 0u;
                bool nhp = true;
                const unsigned diag0 = GL == 16 ? (unsigned)row_shift_up1((int)P[C - 1], (int)wrapv) : (unsigned)shift_up1((int)P[C - 1], (int)wrapv);
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const unsigned diag = c == 0 ? diag0 : P[c - 1];
                    const unsigned upv = P[c];
                    const bool m = ((ubw[c >> 2] >> (8 * (c & 3))) & 0xffu) == xi;
                    const unsigned t1 = u16_sub_sat(diag, MMs), t2 = u16_sub_sat(upv, Ds);
                    const unsigned gnm = u16_max(t1, t2) + Dj[c];
                    const unsigned gm = diag + GDj[c];
                    const unsigned ch = u16_max(gnm, sprev);
                    const unsigned sc = m ? gm : ch;
                    s[c] = sc; t1s[c] = t1; mt[c] = m;
                    nhp = nhp && !m; nh[c] = nhp;
                    sprev = sc;
                }
                const unsigned long long hm = __ballot(!nhp);
                const unsigned seg = (unsigned)mbcnt(hm >> 1);
                const unsigned S = (GL == 16 ? scan_max_u32_row16((seg << 16) | sprev) : scan_max_u32((seg << 16) | sprev)) & 0xFFFFu;
                const unsigned e = GL == 16 ? (unsigned)row_shift_up1((int)S, 0) : (unsigned)shift_up1((int)S, 0);
                unsigned f[8];
#pragma unroll
                for (int c = C; c < 8; c++) f[c] = 0u;
                unsigned hgp = e;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const unsigned mx = u16_max(s[c], e);
                    const unsigned hg = nh[c] ? mx : s[c];
                    const unsigned H = hg - Dj[c];
                    const unsigned nz = u16_min(H, ONE);
                    const unsigned nx = u16_min(H - t1s[c], SC == 4 ? TWO : ONE);
                    const unsigned nd = u16_min(hg - hgp, SC == 4 ? FOUR : ONE);
                    unsigned fl = SC == 4 ? (nz | nx | nd) : (nz | (nx << 1) | (nd << 2));
                    fl = mt[c] ? EIGHT : fl;
                    f[c] = fl;
                    if (!BKP) {
                        const unsigned q0 = (H << 16) | inv_i;
                        bk[c] = q0 > bk[c] ? q0 : bk[c];
                    }
                    P[c] = H;
                    hgp = hg;
                }
                if (BKP) {
                    const unsigned r0 = (0x7FFFu - (unsigned)i) << 1, r1 = r0 | 1u;
#pragma unroll
                    for (int c = 0; c + 1 < C; c += 2) {
                        const unsigned a0 = (P[c] << 16) | r1, b0 = (P[c + 1] << 16) | r0;
                        bk[c >> 1] = max3_u32(bk[c >> 1], a0, b0);
                    }
                    if (C & 1) {
                        const unsigned a0 = (P[C - 1] << 16) | r1;
                        bk[C >> 1] = a0 > bk[C >> 1] ? a0 : bk[C >> 1];
                    }
                }
                unsigned hsel = P[0];
#pragma unroll
                for (int c = 1; c < C; c++) hsel = is_r[c] ? P[c] : hsel;
                // (one DP on the whole wavefront: the lane that holds column U is the same for every lane - a v_readlane instead of the LDS crossbar's
                //  round trip, which sits on the row's critical path: H(i, U) is the next row's first diagonal)
                wrapv = GL == 64 ? (unsigned)__builtin_amdgcn_readlane((int)hsel, lUs) : (unsigned)__builtin_amdgcn_ds_bpermute(hu_addr, (int)hsel);
                {
                    const unsigned nd0 = u16_min(u16_sub(P[0] + Ds, wrapv), SC == 4 ? FOUR : ONE) << (SC == 4 ? 0 : 2);
                    const unsigned f0 = (f[0] & ~4u) | nd0;
                    f[0] = (lane0 && !mt[0]) ? f0 : f[0];
                }
                const unsigned lo = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24);
                const unsigned hi = C > 4 ? f[4] | (f[5] << 8) | (f[6] << 16) | (f[7] << 24) : 0u;
                if (!PAIR) store_cells(lo, hi);
                else if (i & 1) { loP = lo; hiP = hi; }                  // (i is a scalar: the odd row only parks its cells)
                else store_cells(loP | (lo << 4), hiP | (hi << 4));
                loop_join();
            }
            loop_join();
        }
        loop_join();
    }
    if (PAIR && (maxrows & 1)) store_cells(loP, hiP);           // the last row has no partner
    {
        int v = 0, vi = 0, vj = 0;
#pragma unroll
        for (int t = 0; t < NBK; t++) {
            const int c = BKP ? 2 * t + 1 - (int)(bk[t] & 1u) : t;
            const int j = l * C + c + 1;
            const int bvc = (int)(bk[t] >> 16), bic = BKP ? (int)(0x7FFFu - ((bk[t] & 0xFFFFu) >> 1)) : (int)(0xFFFFu - (bk[t] & 0xFFFFu));
            if (j <= Ul && (bvc > v || (bvc == v && bvc > 0 && bic < vi))) { v = bvc; vi = bic; vj = j; }
        }
        for (int dd = GL / 2; dd > 0; dd >>= 1) {
            const int ov = __shfl_xor(v, dd, 64), oi = __shfl_xor(vi, dd, 64), oj = __shfl_xor(vj, dd, 64);
            const bool take = (ov > v) || (ov == v && ov > 0 && (oi < vi || (oi == vi && oj < vj)));
            if (take) { v = ov; vi = oi; vj = oj; }
        }
#pragma unroll
        for (int h = 0; h < NG; h++) { best[h][0] = lane_val(v, GL * h) / SC; best[h][1] = lane_val(vi, GL * h); best[h][2] = lane_val(vj, GL * h); }
    }
}


// ---- EIGHT one-parameter DPs per wavefront (round 5): two DIFFERENT DPs in the 16-bit halves of every register ----------------------------
// dp_forward1p_g16 spends per cell what dp_forward2p_g16 spends per cell PAIR: a 32-bit register carries one 16-bit score.  Here DP 2g lives in the
// low halves and DP 2g + 1 in the high halves of lane group g's registers (same geometry: C columns per lane, 16 lanes; each DP its own unit, window,
// rows and scores): the recurrence runs on v_pk_* (one instruction = both DPs) and on plain 32-bit adds where no carry can cross the halves.  What
// differs per half is made per half WITHOUT per-half instructions:
//   match       x = (unit bases of the column, one per half) ^ (read bases of the row, one per half) is 0 in a half that matches; (x - 1) >> 15
//               (v_pk_sub_u16, v_pk_ashrrev_i16) is then a mask of all ones in that half - two packed instructions for both DPs, where the four-per-wavefront
//               pass takes a byte compare per DP;
//   selects     v_bfi_b32 with such masks ("take the match value in the halves that match"): one instruction for both DPs; the "no match so far in this
//               lane" masks are the running AND of the inverted match masks;
//   H(i, U)     columns U of the two DPs sit in different registers / lanes: a v_bfi chain with per-lane constant masks picks both at once, two
//               ds_bpermute fetch them from the two lanes.
// Cells: as dp_forward1p_g16<., 16, ., true> - every DP its own matrix, two rows per byte row (DPQP_DP_BYTES), read by dp_traceback<., 3>; a match cell
// carries its flag (bit 3) OR-ed over whatever the three other flags came out as (the traceback tests bit 3 first).  Scores times four, as there.
struct DpOct {
    const uint32_t *pk[8]; long long wlim[8]; int base[8], rows[8], U[8]; const uint8_t *unit[8];
    int n;                      // DPs present (1..8); DP d = half d & 1 of lane group d >> 1
    int G[8], MM[8], D[8];
};
DEVINL unsigned v_bfi(unsigned mask, unsigned a, unsigned b) { unsigned r; asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(a), "v"(b)); return r; }     // (mask & a) | (~mask & b)
DEVINL unsigned pk_ashr15(unsigned a) { unsigned r; asm("v_pk_ashrrev_i16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(r) : "v"(a)); return r; }                             // per half: all ones if bit 15 is set
DEVINL unsigned v_and_or(unsigned a, unsigned b, unsigned c) { unsigned r; asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }   // (a & b) | c
template <int C>
DEVINL void dp_forward1p_h8(const DpOct &q, uint8_t *cells, int maxrows, int (&best)[8][3])
{
    static_assert(C >= 1 && C <= 8, "columns per lane");
    constexpr int SC = DPQ_SCALE;
    const int lane = lane_id();
    const int g = lane >> 4, l = lane & 15;
    unsigned ONE = 0x00010001u, TWO = 0x00020002u, FOUR = 0x00040004u, C8 = 0x00080008u, LOH = 0x0000FFFFu;
    asm volatile("" : "+v"(ONE), "+v"(TWO), "+v"(FOUR), "+v"(C8), "+v"(LOH));
    // ---- this lane's two DPs: A = 2g (low halves), B = 2g + 1 (high halves)
    int Ua = 0, Ub = 0, basea = 0, baseb = 0, rowsa = 0, rowsb = 0, Ga = 1, Gb = 1, MMa = 1, MMb = 1, Da = 1, Db = 1;
    const uint8_t *upa = q.unit[0], *upb = q.unit[0]; const uint32_t *pka = q.pk[0], *pkb = q.pk[0]; long long wla = 1, wlb = 1;
#pragma unroll
    for (int h = 0; h < 4; h++) if (g == h) {
        Ua = q.U[2 * h]; basea = q.base[2 * h]; rowsa = q.rows[2 * h]; upa = q.unit[2 * h]; pka = q.pk[2 * h]; wla = q.wlim[2 * h]; Ga = q.G[2 * h]; MMa = q.MM[2 * h]; Da = q.D[2 * h];
        Ub = q.U[2 * h + 1]; baseb = q.base[2 * h + 1]; rowsb = q.rows[2 * h + 1]; upb = q.unit[2 * h + 1]; pkb = q.pk[2 * h + 1]; wlb = q.wlim[2 * h + 1]; Gb = q.G[2 * h + 1]; MMb = q.MM[2 * h + 1]; Db = q.D[2 * h + 1];
    }
    if (2 * g >= q.n) { Ua = 0; rowsa = 0; }
    if (2 * g + 1 >= q.n) { Ub = 0; rowsb = 0; }
    const unsigned Gpk = SC * ((unsigned)Ga | ((unsigned)Gb << 16)), MMpk = SC * ((unsigned)MMa | ((unsigned)MMb << 16)), Dpk = SC * ((unsigned)Da | ((unsigned)Db << 16));
    // per column: the two unit bases (4 = no such column: no read base equals it), the chain constants D j and D j + G (j = the DP's column, from 1), and the
    // mask of the halves whose column U this register is
    const int lUa = Ua > 0 ? (Ua - 1) / C : 0, rUa = Ua > 0 ? (Ua - 1) % C : 0, lUb = Ub > 0 ? (Ub - 1) / C : 0, rUb = Ub > 0 ? (Ub - 1) % C : 0;
    unsigned ubc[C], Dj[C], GDj[C], isr[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int j = l * C + c + 1;
        const unsigned ba = j <= Ua && rowsa > 0 ? (unsigned)(upa[j - 1] & 3) : 4u, bb = j <= Ub && rowsb > 0 ? (unsigned)(upb[j - 1] & 3) : 4u;
        ubc[c] = ba | (bb << 16);
        Dj[c] = SC * ((unsigned)(Da * j) | ((unsigned)(Db * j) << 16));
        GDj[c] = Dj[c] + Gpk;
        isr[c] = (rUa == c ? 0x0000FFFFu : 0u) | (rUb == c ? 0xFFFF0000u : 0u);
    }
    {
        int landed = lane_val((int)(ubc[0] ^ ubc[C - 1]), 0);
        asm volatile("" :: "s"(landed));
    }
    const int hua_addr = (g * 16 + lUa) << 2, hub_addr = (g * 16 + lUb) << 2;
    const bool lane0 = l == 0;
    const int grp_addr = (g * 16) << 2;
    constexpr int NBK = (C + 1) / 2;                            // best cell per column pair and DP (as dp_forward1p_g16: key = H << 16 | (0x7FFF - i) << 1 | first of the pair)
    unsigned P[C], bka[NBK], bkb[NBK];
#pragma unroll
    for (int c = 0; c < C; c++) P[c] = 0u;
#pragma unroll
    for (int c = 0; c < NBK; c++) { bka[c] = 0u; bkb[c] = 0u; }
    unsigned wrapv = 0u;
    int next_done = maxrows + 1;
#pragma unroll
    for (int h = 0; h < 8; h++) { const int r = h < q.n ? q.rows[h] : 0; if (r < next_done) next_done = r; }
    const size_t mbytes = DPQP_DP_BYTES(C, maxrows);
    uint8_t *crowa = cells + (size_t)(2 * g) * mbytes + (size_t)l * C, *crowb = crowa + mbytes;
    unsigned loPa = 0u, hiPa = 0u, loPb = 0u, hiPb = 0u;         // the odd row's packed cells, waiting for the even row
    const bool has_a = 2 * g < q.n, has_b = 2 * g + 1 < q.n;
    auto store_cells = [&](uint8_t *crow, unsigned lo, unsigned hi, bool present) {
        if (C > 4) {
            if (C < 8) {
                const unsigned nlo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x130, 0xf, 0xf, false);
                hi |= nlo << (8 * (C > 4 && C < 8 ? C - 4 : 0));
            }
            if (present) *(uint2 *)crow = make_uint2(lo, hi);
        } else if (C == 1) {
            if (present) *crow = (uint8_t)lo;
        } else {
            if (C < 4) {
                const unsigned nlo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x130, 0xf, 0xf, false);
                lo |= nlo << (8 * (C < 4 ? C : 0));
            }
            if (present) *(uint32_t *)crow = lo;
        }
    };
    int i = 1;
    constexpr int CHUNK = 16 * 16 - 16;
    for (int t0 = 0; t0 < maxrows; t0 += CHUNK) {
        // ---- stage the chunk's windows: lane l holds 16 bases of each of its two DPs, first base in bit 30
        uint32_t Aw, Bw;
        {
            const int pos0 = basea + 1 + t0;
            long long w0 = (long long)(pos0 >> 4) + l, w1 = w0 + 1;
            if (w0 > wla - 1) w0 = wla - 1;
            if (w1 > wla - 1) w1 = wla - 1;
            if (w0 < 0) w0 = 0;
            if (w1 < 0) w1 = 0;
            const uint32_t wa = pka[w0], wb = pka[w1];
            Aw = (uint32_t)(((((unsigned long long)wa) << 32) | (unsigned long long)wb) >> (32u - 2u * (unsigned)(pos0 & 15)));
        }
        {
            const int pos0 = baseb + 1 + t0;
            long long w0 = (long long)(pos0 >> 4) + l, w1 = w0 + 1;
            if (w0 > wlb - 1) w0 = wlb - 1;
            if (w1 > wlb - 1) w1 = wlb - 1;
            if (w0 < 0) w0 = 0;
            if (w1 < 0) w1 = 0;
            const uint32_t wa = pkb[w0], wb = pkb[w1];
            Bw = (uint32_t)(((((unsigned long long)wa) << 32) | (unsigned long long)wb) >> (32u - 2u * (unsigned)(pos0 & 15)));
        }
        {
            int landed = lane_val((int)(Aw ^ Bw), 0);
            asm volatile("" :: "s"(landed));
        }
        const int i_chunk_end = t0 + CHUNK < maxrows ? t0 + CHUNK : maxrows;
        for (int wd = 0; i <= i_chunk_end; wd++) {
            const uint32_t wcura = (uint32_t)__builtin_amdgcn_ds_bpermute(grp_addr + (wd << 2), (int)Aw);
            const uint32_t wcurb = (uint32_t)__builtin_amdgcn_ds_bpermute(grp_addr + (wd << 2), (int)Bw);
            // the 16 rows' bases of both DPs side by side, two bits each: base of row t at bits 30 - 2t (A) and of B sixteen bits up, after the shift below
            const int i_w_end = i + 15 < i_chunk_end ? i + 15 : i_chunk_end;
            int bsh = 30;
#pragma unroll 1
            for (; i <= i_w_end; i++, bsh -= 2) {
                if (i > next_done) {                            // rare: some DP of the wavefront has had its last row: it goes on with "nothing matches"
                    asm volatile("; a DP of the pass has ended" ::: "memory");       // (keeps this a branch: if-converted it is 2 C selects in every row)
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        if (i > rowsa) ubc[c] = (ubc[c] & 0xFFFF0000u) | 4u;
                        if (i > rowsb) ubc[c] = (ubc[c] & 0x0000FFFFu) | (4u << 16);
                    }
                    next_done = maxrows + 1;
#pragma unroll
                    for (int h = 0; h < 8; h++) { const int r = h < q.n ? q.rows[h] : 0; if (r >= i && r < next_done) next_done = r; }
                }
                const unsigned xi = lshl_or<16>(__builtin_amdgcn_ubfe(wcurb, (unsigned)bsh, 2u), __builtin_amdgcn_ubfe(wcura, (unsigned)bsh, 2u));
                // ---- phase A: the lane's own chains, as if nothing came in from the left
                unsigned s[C], t1s[C], mk[C];
                unsigned sprev = 0u, many = 0u;
                const unsigned diag0 = (unsigned)row_shift_up1((int)P[C - 1], (int)wrapv);
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const unsigned diag = c == 0 ? diag0 : P[c - 1];
                    const unsigned upv = P[c];
                    const unsigned m = pk_ashr15(pk_sub(ubc[c] ^ xi, ONE));          // all ones in the halves whose bases match
                    const unsigned t1 = pk_sub_sat(diag, MMpk), t2 = pk_sub_sat(upv, Dpk);
                    const unsigned gnm = pk_max(t1, t2) + Dj[c];                       // no carry between the halves: plain adds
                    const unsigned gm = diag + GDj[c];
                    const unsigned ch = pk_max(gnm, sprev);
                    const unsigned sc = v_bfi(m, gm, ch);
                    many |= m;
                    s[c] = sc; t1s[c] = t1; mk[c] = m;
                    sprev = sc;
                }
                // ---- what arrives from the left, per DP: segmented prefix maximum over the group's 16 lanes of the value leaving each lane
                const unsigned long long hma = __ballot((many & 0x0000FFFFu) != 0u), hmb = __ballot((many >> 16) != 0u);      // lanes that hold a match, per DP
                const unsigned sega = (unsigned)mbcnt(hma >> 1), segb = (unsigned)mbcnt(hmb >> 1);
                unsigned k0 = lshl_or<16>(sega, sprev & LOH);
                unsigned k1 = lshl_or<16>(segb, sprev >> 16);
                scan_max_u32_x2_row16(k0, k1);
                const unsigned S = lshl_or<16>(k1, k0 & LOH);
                const unsigned e = (unsigned)row_shift_up1((int)S, 0);
                // ---- phase B: the incoming value reaches the columns before the lane's first match
                unsigned f[8];
#pragma unroll
                for (int c = C; c < 8; c++) f[c] = 0u;
                unsigned hgp = e, erun = e;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    erun = v_bfi(mk[c], 0u, erun);                                     // nothing comes in past a match (per half)
                    const unsigned hg = pk_max(s[c], erun);
                    const unsigned H = hg - Dj[c];
                    const unsigned nz = pk_nonzero(H, ONE);
                    const unsigned nx = pk_nonzero(H - t1s[c], TWO);                   // H >= t1 in a non-match half; a match half is overridden below
                    const unsigned nd = pk_nonzero(pk_sub(hg, hgp), FOUR);             // (pk: a match half may have hg < hgp - the borrow must not reach the other DP)
                    unsigned fl;
                    asm("v_or3_b32 %0, %1, %2, %3" : "=v"(fl) : "v"(nz), "v"(nx), "v"(nd));
                    f[c] = v_and_or(mk[c], C8, fl);
                    P[c] = H;
                    hgp = hg;
                }
                {
                    const unsigned r0 = (0x7FFFu - (unsigned)i) << 1, r1 = r0 | 1u;
#pragma unroll
                    for (int c = 0; c + 1 < C; c += 2) {
                        bka[c >> 1] = max3_u32(bka[c >> 1], (P[c] << 16) | r1, (P[c + 1] << 16) | r0);
                        bkb[c >> 1] = max3_u32(bkb[c >> 1], (P[c] & 0xFFFF0000u) | r1, (P[c + 1] & 0xFFFF0000u) | r0);
                    }
                    if (C & 1) {
                        const unsigned a0 = (P[C - 1] << 16) | r1, b0 = (P[C - 1] & 0xFFFF0000u) | r1;
                        bka[C >> 1] = a0 > bka[C >> 1] ? a0 : bka[C >> 1];
                        bkb[C >> 1] = b0 > bkb[C >> 1] ? b0 : bkb[C >> 1];
                    }
                }
                // ---- H(i,U) of both DPs: next row's wrap, and column 1's "left" in the traceback's deletion test (:302/:314)
                unsigned hsel = P[0];
#pragma unroll
                for (int c = 1; c < C; c++) hsel = v_bfi(isr[c], P[c], hsel);
                {
                    const unsigned wa = (unsigned)__builtin_amdgcn_ds_bpermute(hua_addr, (int)hsel), wb = (unsigned)__builtin_amdgcn_ds_bpermute(hub_addr, (int)hsel);
                    wrapv = v_bfi(LOH, wa, wb);
                }
                {
                    const unsigned nd0 = pk_nonzero(pk_sub(pk_add(P[0], Dpk), wrapv), FOUR);
                    const unsigned f0 = (f[0] & ~0x00040004u) | nd0;
                    f[0] = lane0 ? v_bfi(mk[0], f[0], f0) : f[0];
                }
                // ---- cells: per DP, byte c = the lane's c-th cell (flags in the low nibble); two rows per byte row
                const unsigned F01 = lshl_or<8>(f[1], f[0]), F23 = lshl_or<8>(f[3], f[2]);
                const unsigned loa = __builtin_amdgcn_perm(F23, F01, 0x05040100u), lob = __builtin_amdgcn_perm(F23, F01, 0x07060302u);
                unsigned hia = 0u, hib = 0u;
                if (C > 4) {
                    const unsigned F45 = C > 5 ? lshl_or<8>(f[5], f[4]) : f[4], F67 = C > 7 ? lshl_or<8>(f[7], f[6]) : f[6];
                    hia = __builtin_amdgcn_perm(F67, F45, 0x05040100u); hib = __builtin_amdgcn_perm(F67, F45, 0x07060302u);
                }
                if (i & 1) { loPa = loa; hiPa = hia; loPb = lob; hiPb = hib; }       // (i is a scalar: the odd row only parks its cells)
                else {
                    // (a DP that is not there - a pass of 5..7 members - writes nothing; the neighbour-lane exchange inside runs for every lane)
                    store_cells(crowa, lshl_or<4>(loa, loPa), C > 4 ? lshl_or<4>(hia, hiPa) : 0u, has_a);
                    store_cells(crowb, lshl_or<4>(lob, loPb), C > 4 ? lshl_or<4>(hib, hiPb) : 0u, has_b);
                    crowa += DPQ_ROW_BYTES(C); crowb += DPQ_ROW_BYTES(C);
                }
                loop_join();
            }
            loop_join();
        }
        loop_join();
    }
    if (maxrows & 1) { store_cells(crowa, loPa, hiPa, has_a); store_cells(crowb, loPb, hiPb, has_b); }     // the last row has no partner
    // ---- best cell per DP: largest value, then smallest i, then smallest j
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const int Ud = d == 0 ? Ua : Ub;
        int v = 0, vi = 0, vj = 0;
#pragma unroll
        for (int t = 0; t < NBK; t++) {
            const unsigned bk = d == 0 ? bka[t] : bkb[t];
            const int c = 2 * t + 1 - (int)(bk & 1u);
            const int j = l * C + c + 1;
            const int bvc = (int)(bk >> 16), bic = (int)(0x7FFFu - ((bk & 0xFFFFu) >> 1));
            if (j <= Ud && (bvc > v || (bvc == v && bvc > 0 && bic < vi))) { v = bvc; vi = bic; vj = j; }
        }
        for (int dd = 8; dd > 0; dd >>= 1) {
            const int ov = __shfl_xor(v, dd, 64), oi = __shfl_xor(vi, dd, 64), oj = __shfl_xor(vj, dd, 64);
            const bool take = (ov > v) || (ov == v && ov > 0 && (oi < vi || (oi == vi && oj < vj)));
            if (take) { v = ov; vi = oi; vj = oj; }
        }
#pragma unroll
        for (int h = 0; h < 4; h++) { best[2 * h + d][0] = lane_val(v, 16 * h) / SC; best[2 * h + d][1] = lane_val(vi, 16 * h); best[2 * h + d][2] = lane_val(vj, 16 * h); }
    }
}
