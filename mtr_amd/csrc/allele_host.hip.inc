// allele_host.hip.inc — the hosts of what follows a genotype, included by mtr_abi.hip below genotype_host.hip.inc: the allele calls, the windows and
// the allele consensus, the motif structure of windows.  Every one takes the caller's device columns: they are checked by check_device_cols, and
// the context's stream waits for the caller's (wait_for_stream) before a kernel reads them.

// ---- allele calls (allele_call.hip.inc) ------------------------------------------------------------------------------------------------
// The arguments' checks, the count and the offsets, one look at the device (the status, S, the tiles), then the fill, the rank and the split
// straight into the caller's columns.  No batch is needed and none is touched.
// rows: the four input columns with R rows; row_read / row_locus: NULL for the dense layout (row = read * n_loci + locus), else the rows' own
static mtr_status call_alleles_rows(mtr_ctx *ctx, const mtr_genotypes_dst *rows, int64_t R, int32_t n_loci, const int32_t *row_read, const int32_t *row_locus,
                                    const mtr_allele_params *prm, void *wait_stream, const mtr_allele_calls_dst *dst, int64_t *out_support)
{
    if (prm->measure != MTR_ALLELE_COPIES && prm->measure != MTR_ALLELE_BASES) { ctx->err = "measure " + std::to_string(prm->measure) + " is neither MTR_ALLELE_COPIES nor MTR_ALLELE_BASES"; return MTR_ERR_BAD_ARG; }
    if (!(prm->min_ratio >= 0.0f && prm->min_ratio <= 1.0f)) { ctx->err = "min_ratio " + std::to_string(prm->min_ratio) + " outside 0..1"; return MTR_ERR_BAD_ARG; }
    if (prm->min_support < 1) { ctx->err = "min_support " + std::to_string(prm->min_support) + ": at least 1"; return MTR_ERR_BAD_ARG; }
    if (prm->min_percent < 0 || prm->min_percent > 50) { ctx->err = "min_percent " + std::to_string(prm->min_percent) + " outside 0..50"; return MTR_ERR_BAD_ARG; }
    if (prm->min_sep < 1) { ctx->err = "min_sep " + std::to_string(prm->min_sep) + ": at least 1"; return MTR_ERR_BAD_ARG; }
    if (R > 0 && (!rows->spanning || !rows->window || !rows->fields || !rows->ratio)) { ctx->err = "an input column (spanning, window, fields, ratio) is NULL"; return MTR_ERR_BAD_ARG; }
    if (rows->cap_rows < R) { ctx->err = "cap_rows " + std::to_string(rows->cap_rows) + " of the input is below " + std::to_string(R) + " rows"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t own = row_locus ? R * 4 : 0;                                                          // the dense layout has no index columns
    const DeviceCol cols[6] = { { rows->spanning, R, "rows->spanning" }, { rows->window, R * 8, "rows->window" }, { rows->fields, R * 32, "rows->fields" },
                                { rows->ratio, R * 4, "rows->ratio" }, { row_read, own, "row_read" }, { row_locus, own, "row_locus" } };
    { mtr_status st = check_device_cols(ctx, cols, "the rows' bytes"); if (st != MTR_OK) return st; }
    const size_t nl = (size_t)n_loci;
    const size_t cstride = n_loci <= AL_SPREAD_LOCI ? AL_SPREAD : 1;
    HIPCHK(ctx->d_ac_i32.ensure(2 * nl * cstride * 4)); HIPCHK(ctx->d_ac_i64.ensure((2 * (nl + 1) + AL_STATE) * 8));
    AlleleArgs a{};
    a.spanning = rows->spanning; a.window = rows->window; a.fields = rows->fields; a.ratio = rows->ratio;
    a.row_read = R > 0 ? row_read : nullptr; a.row_locus = R > 0 ? row_locus : nullptr;
    a.rows = R; a.n_loci = n_loci; a.measure = prm->measure; a.min_ratio = prm->min_ratio; a.rule = { prm->min_support, prm->min_percent, prm->min_sep };
    a.count = ctx->d_ac_i32; a.cursor = a.count + nl * cstride; a.cstride = (int32_t)cstride; a.off = ctx->d_ac_i64; a.tile_off = a.off + nl + 1; a.state = a.tile_off + nl + 1;
    { mtr_status st = wait_for_stream(ctx, wait_stream); if (st != MTR_OK) return st; }               // the rows come from the caller's stream
    if (a.row_locus) {
        // the index columns before anything else reads them: every locus in range, every (locus, read) once - the rank's keys are distinct by that
        unsigned long long cap = 64; while (cap < 2 * (unsigned long long)R) cap <<= 1;
        HIPCHK(ctx->d_ac_keys.ensure((size_t)(cap + 2) * 8));
        unsigned long long *set = ctx->d_ac_keys, *bad = set + cap;
        HIPCHK(hipMemsetAsync(set, 0xff, (size_t)(cap + 2) * 8, ctx->stream));
        hipLaunchKernelGGL(mtr_k_cat_rows_check, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, ctx->stream, row_read, row_locus, R, n_loci, set, cap, bad);
        HIPCHK(hipGetLastError());
        unsigned long long found[2];
        HIPCHK(copy_sync(ctx, found, bad, sizeof found, hipMemcpyDeviceToHost));
        if (found[0] != ~0ull) {
            int32_t rl[2] = { 0, 0 };
            HIPCHK(copy_sync(ctx, &rl[0], row_read + found[0], 4, hipMemcpyDeviceToHost)); HIPCHK(copy_sync(ctx, &rl[1], row_locus + found[0], 4, hipMemcpyDeviceToHost));
            ctx->err = "row " + std::to_string(found[0]) + ": read " + std::to_string(rl[0]) + " is negative or locus " + std::to_string(rl[1]) + " is outside 0.." + std::to_string(n_loci - 1);
            return MTR_ERR_BAD_ARG;
        }
        if (found[1] != ~0ull) {
            ctx->err = "(locus " + std::to_string(found[1] >> 32) + ", read " + std::to_string(found[1] & 0xffffffffull) + ") is given by more than one row";
            return MTR_ERR_BAD_ARG;
        }
    }
    HIPCHK(hipMemsetAsync(ctx->d_ac_i32, 0, 2 * nl * cstride * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(a.state, 0xff, 8, ctx->stream));
    const dim3 per_row((unsigned)((R + AL_BLOCK - 1) / AL_BLOCK)), blk(AL_BLOCK);
    if (R > 0) hipLaunchKernelGGL(mtr_k_allele_count, per_row, blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mtr_k_allele_offsets, dim3(1), dim3(64), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    int64_t st[AL_STATE];
    HIPCHK(copy_sync(ctx, st, a.state, 3 * 8, hipMemcpyDeviceToHost));
    const int64_t S = st[AL_TOTAL], n_tiles = st[AL_TILES];
    if (S < 0 || S > R || n_tiles < 0 || n_tiles > S) { ctx->err = "the allele calls' count failed on the device"; return MTR_ERR_HIP; }
    *out_support = S;
    if (st[AL_BAD] != -1) {
        const int64_t p = st[AL_BAD];
        int64_t rd = p / n_loci, l = p % n_loci;
        if (a.row_locus) {
            int32_t rl[2] = { 0, 0 };
            HIPCHK(copy_sync(ctx, &rl[0], row_read + p, 4, hipMemcpyDeviceToHost)); HIPCHK(copy_sync(ctx, &rl[1], row_locus + p, 4, hipMemcpyDeviceToHost));
            rd = rl[0]; l = rl[1];
        }
        ctx->err = "row " + std::to_string(p) + " (read " + std::to_string(rd) + ", locus " + std::to_string(l) + ") supports its locus with a negative value";
        return MTR_ERR_BAD_ARG;
    }
    if (!dst) return MTR_OK;
    if (dst->cap_loci < n_loci) { ctx->err = "destination holds " + std::to_string(dst->cap_loci) + " loci, " + std::to_string(n_loci) + " needed"; return MTR_ERR_OVERFLOW; }
    if (dst->cap_support < S) { ctx->err = "destination holds " + std::to_string(dst->cap_support) + " supporting rows, " + std::to_string(S) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->support_off || !dst->zygosity || !dst->call || !dst->call_support || !dst->cost || (S > 0 && (!dst->value || !dst->read || !dst->allele))) {
        ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG;
    }
    HIPCHK(ctx->d_ac_keys.ensure((size_t)std::max<int64_t>(S, 1) * 8)); HIPCHK(ctx->d_ac_prefix.ensure(((size_t)S + nl) * 8));
    a.keys = ctx->d_ac_keys; a.prefix = ctx->d_ac_prefix;
    a.value = dst->value; a.read = dst->read; a.allele = dst->allele; a.zygosity = dst->zygosity; a.call = dst->call; a.call_support = dst->call_support; a.cost = dst->cost;
    if (S > 0) {
        hipLaunchKernelGGL(mtr_k_allele_fill, per_row, blk, 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mtr_k_allele_rank, dim3((unsigned)std::min<int64_t>(n_tiles, AL_MAX_GRID)), dim3(AL_TILE), 0, ctx->stream, a, n_tiles);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mtr_k_allele_split, dim3((unsigned)std::min<int64_t>(n_loci, AL_MAX_GRID)), blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst->support_off, a.off, (nl + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

extern "C" mtr_status mtr_call_alleles_device(mtr_ctx *ctx, const mtr_genotypes_dst *rows, int64_t n_reads, int32_t n_loci, const mtr_allele_params *prm,
                                              void *wait_stream, const mtr_allele_calls_dst *dst, int64_t *out_support)
{
    if (!ctx || !out_support) return MTR_ERR_BAD_ARG;
    *out_support = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (!rows || !prm) { ctx->err = "rows or prm is NULL"; return MTR_ERR_BAD_ARG; }
    if (n_reads < 1) { ctx->err = "n_reads = " + std::to_string(n_reads) + ": at least one read is needed"; return MTR_ERR_BAD_ARG; }
    if (n_loci < 1) { ctx->err = "n_loci = " + std::to_string(n_loci) + ": at least one locus is needed"; return MTR_ERR_BAD_ARG; }
    if (n_reads > (int64_t)INT32_MAX / n_loci) { ctx->err = std::to_string(n_reads) + " reads x " + std::to_string(n_loci) + " loci are more than 2^31 - 1 rows"; return MTR_ERR_BAD_ARG; }
    return call_alleles_rows(ctx, rows, n_reads * n_loci, n_loci, nullptr, nullptr, prm, wait_stream, dst, out_support);
}

extern "C" mtr_status mtr_call_alleles_rows_device(mtr_ctx *ctx, const mtr_genotypes_dst *rows, const int32_t *row_read, const int32_t *row_locus, int64_t n_rows,
                                                   int32_t n_loci, const mtr_allele_params *prm, void *wait_stream, const mtr_allele_calls_dst *dst, int64_t *out_support)
{
    if (!ctx || !out_support) return MTR_ERR_BAD_ARG;
    *out_support = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (!rows || !prm) { ctx->err = "rows or prm is NULL"; return MTR_ERR_BAD_ARG; }
    if (n_rows < 0 || n_rows > (int64_t)INT32_MAX) { ctx->err = "n_rows = " + std::to_string(n_rows) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (n_loci < 1) { ctx->err = "n_loci = " + std::to_string(n_loci) + ": at least one locus is needed"; return MTR_ERR_BAD_ARG; }
    if (n_rows > 0 && (!row_read || !row_locus)) { ctx->err = "row_read or row_locus is NULL"; return MTR_ERR_BAD_ARG; }
    return call_alleles_rows(ctx, rows, n_rows, n_loci, row_read, row_locus, prm, wait_stream, dst, out_support);
}

// ---- windows and allele consensus (consensus.hip.inc) ------------------------------------------------------------------------------------
// the caller's stream before the context's, and a call's state words: n_bad bad-input words set to "none", zero_bytes of counters behind them to 0
static mtr_status columns_begin(mtr_ctx *ctx, void *wait_stream, DevBuf<unsigned long long> &state, size_t n_bad, size_t zero_bytes)
{
    HIPCHK(state.ensure(n_bad * 8 + zero_bytes));
    { mtr_status st = wait_for_stream(ctx, wait_stream); if (st != MTR_OK) return st; }
    HIPCHK(hipMemsetAsync(state, 0xff, n_bad * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(state + n_bad, 0, zero_bytes, ctx->stream));
    return MTR_OK;
}

// what the windows and their qualities share, up to the windows' offsets on the device (ctx->d_co_i64, [n_rows + 1]) and *out_bases = T
static mtr_status windows_front(mtr_ctx *ctx, const int32_t *row_read, const uint8_t *orientation, const int32_t *window, int64_t n_rows, void *wait_stream, bool qualities,
                                int64_t *out_bases)
{
    if (!ctx || !out_bases) return MTR_ERR_BAD_ARG;
    *out_bases = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    if (qualities && ctx->qual_bytes <= 0) { ctx->err = "no qualities resident"; return MTR_ERR_BAD_ARG; }
    const int64_t R = n_rows;
    if (R < 0 || R > (int64_t)INT32_MAX) { ctx->err = "n_rows = " + std::to_string(R) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (R > 0 && (!row_read || !orientation || !window)) { ctx->err = "row_read, orientation or window is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const DeviceCol cols[3] = { { row_read, R * 4, "row_read" }, { orientation, R, "orientation" }, { window, R * 8, "window" } };
    { mtr_status st = check_device_cols(ctx, cols, "the rows' bytes"); if (st != MTR_OK) return st; }
    const size_t nr = (size_t)R;
    HIPCHK(ctx->d_co_i32.ensure(std::max<size_t>(nr, 1) * 4)); HIPCHK(ctx->d_co_i64.ensure((nr + 1) * 8));
    { mtr_status st = columns_begin(ctx, wait_stream, ctx->d_co_state, CO_BAD, CO_STATE * 8); if (st != MTR_OK) return st; }
    unsigned long long *bad = ctx->d_co_state;
    int32_t *len = ctx->d_co_i32; int64_t *off = ctx->d_co_i64;
    if (R > 0) hipLaunchKernelGGL(mtr_k_win_len, dim3((unsigned)((R + CO_BLOCK - 1) / CO_BLOCK)), dim3(CO_BLOCK), 0, ctx->stream, row_read, window, R,
                                  (const int32_t *)ctx->d_lens, (int32_t)ctx->n_reads, len, bad);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)len, R, off);
    HIPCHK(hipGetLastError());
    unsigned long long found = 0; int64_t T = 0;
    HIPCHK(hipMemcpyAsync(&T, off + R, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(copy_sync(ctx, &found, bad + 5, 8, hipMemcpyDeviceToHost));
    if (found != ~0ull) {
        int32_t v[3] = { 0, 0, 0 };
        HIPCHK(copy_sync(ctx, &v[0], row_read + found, 4, hipMemcpyDeviceToHost)); HIPCHK(copy_sync(ctx, &v[1], window + 2 * found, 8, hipMemcpyDeviceToHost));
        ctx->err = "row " + std::to_string(found) + ": read " + std::to_string(v[0]) + " is outside the batch of " + std::to_string(ctx->n_reads) + " reads, or its window " +
                   std::to_string(v[1]) + ".." + std::to_string(v[2]) + " outside the read";
        return MTR_ERR_BAD_ARG;
    }
    if (T < 0) { ctx->err = "the windows' scan failed on the device"; return MTR_ERR_HIP; }
    *out_bases = T;
    return MTR_OK;
}

extern "C" mtr_status mtr_extract_windows_device(mtr_ctx *ctx, const int32_t *row_read, const uint8_t *orientation, const int32_t *window, int64_t n_rows,
                                                 void *wait_stream, const mtr_windows_dst *dst, int64_t *out_bases)
{
    { mtr_status st = windows_front(ctx, row_read, orientation, window, n_rows, wait_stream, false, out_bases); if (st != MTR_OK) return st; }
    const int64_t R = n_rows, T = *out_bases; const size_t nr = (size_t)R;
    const int64_t *off = ctx->d_co_i64;
    if (!dst) return MTR_OK;
    if (dst->cap_rows < R) { ctx->err = "destination holds " + std::to_string(dst->cap_rows) + " rows, " + std::to_string(R) + " needed"; return MTR_ERR_OVERFLOW; }
    if (dst->cap_bases < T) { ctx->err = "destination holds " + std::to_string(dst->cap_bases) + " bases, " + std::to_string(T) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->win_off || (T > 0 && !dst->win_bases)) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    if (T > 0) {
        hipLaunchKernelGGL(mtr_k_win_gather, dim3((unsigned)std::min<int64_t>(R, CO_MAX_GRID)), dim3(64), 0, ctx->stream, row_read, orientation, window, R,
                           (const uint32_t *)ctx->d_packed, (const int64_t *)ctx->d_woff, off, dst->win_bases);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(dst->win_off, off, (nr + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

extern "C" mtr_status mtr_extract_window_qualities_device(mtr_ctx *ctx, const int32_t *row_read, const uint8_t *orientation, const int32_t *window, int64_t n_rows,
                                                          void *wait_stream, uint8_t *dst_qual, int64_t cap, int64_t *out_bases)
{
    { mtr_status st = windows_front(ctx, row_read, orientation, window, n_rows, wait_stream, true, out_bases); if (st != MTR_OK) return st; }
    const int64_t R = n_rows, T = *out_bases;
    if (!dst_qual) return MTR_OK;
    if (cap < T) { ctx->err = "destination holds " + std::to_string(cap) + " bases, " + std::to_string(T) + " needed"; return MTR_ERR_OVERFLOW; }
    if (T > 0) {
        hipLaunchKernelGGL(mtr_k_win_qual, dim3((unsigned)std::min<int64_t>(R, CO_MAX_GRID)), dim3(64), 0, ctx->stream, row_read, orientation, window, R,
                           (const uint8_t *)ctx->d_qual, (const int64_t *)ctx->d_qual_off, (const int64_t *)ctx->d_co_i64, dst_qual);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- the batch's qualities from the caller (quality.hip.inc) ------------------------------------------------------------------------------------
// the batch's place for them: d_qual_off = the exclusive sum of the resident lengths, d_qual sized for all (+ 4: the last aligned dword); enqueues
static mtr_status qualities_layout(mtr_ctx *ctx, int64_t &total)
{
    const size_t n = (size_t)ctx->n_reads;
    total = 0;
    for (int32_t len : ctx->lens) total += len;
    HIPCHK(ctx->d_qual.ensure((size_t)total + 4)); HIPCHK(ctx->d_qual_off.ensure((n + 1) * 8));
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)ctx->d_lens, (int64_t)n, (int64_t *)ctx->d_qual_off);
    HIPCHK(hipGetLastError());
    return MTR_OK;
}
extern "C" mtr_status mtr_keep_qualities(mtr_ctx *ctx, int32_t on)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    ctx->keep_qual = on != 0;
    return MTR_OK;
}
extern "C" mtr_status mtr_qualities_resident(const mtr_ctx *ctx, int64_t *out_bytes)
{
    if (!ctx || !out_bytes) return MTR_ERR_BAD_ARG;
    *out_bytes = ctx->n_reads > 0 ? ctx->qual_bytes : 0;
    return MTR_OK;
}
extern "C" mtr_status mtr_attach_qualities_device(mtr_ctx *ctx, const uint8_t *d_qual, int64_t n_bytes, const int64_t *offsets, void *wait_stream)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    if (!d_qual || !offsets) { ctx->err = "d_qual or offsets is NULL"; return MTR_ERR_BAD_ARG; }
    if (n_bytes <= 0) { ctx->err = "n_bytes " + std::to_string(n_bytes) + " <= 0"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    { mtr_status st = check_device_ptr(ctx, d_qual, n_bytes, "d_qual", "n_bytes"); if (st != MTR_OK) return st; }
    const size_t n = (size_t)ctx->n_reads;
    for (size_t i = 0; i < n; i++)
        if (offsets[i] < 0 || offsets[i] > n_bytes - ctx->lens[i]) {
            ctx->err = "read " + std::to_string(i) + ": values " + std::to_string(offsets[i]) + " .. +" + std::to_string(ctx->lens[i]) + " outside d_qual's " + std::to_string(n_bytes) + " bytes";
            return MTR_ERR_BAD_ARG;
        }
    HIPCHK(ctx->d_toff.ensure(n * 8));
    HIPCHK(copy_sync(ctx, ctx->d_toff, offsets, n * 8, hipMemcpyHostToDevice));
    { mtr_status st = wait_for_stream(ctx, wait_stream); if (st != MTR_OK) return st; }               // the values come from the caller's stream
    ctx->qual_bytes = 0;                                                                                // (what was there is being overwritten)
    int64_t total = 0;
    { mtr_status st = qualities_layout(ctx, total); if (st != MTR_OK) return st; }
    hipLaunchKernelGGL(mtr_k_qual_gather<false>, dim3((unsigned)std::min<int64_t>(ctx->n_reads, QL_MAX_GRID)), dim3(64), 0, ctx->stream, d_qual, (const uint32_t *)nullptr,
                       (const int64_t *)ctx->d_toff, (const int32_t *)ctx->d_lens, (const int64_t *)ctx->d_qual_off, (int32_t)ctx->n_reads, (uint8_t *)ctx->d_qual);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->qual_bytes = total;
    return MTR_OK;
}

// one bucket's alignments: the grid is bounded by the scratch it may take (each wavefront its own directions, sized by the bucket's longest task)
// qual: the weighted vote's two arguments, NULL for the unweighted one
struct ConsWeights { const uint8_t *win_qual; int32_t qual_cap; };
template <int CPL>
static mtr_status cons_align_bucket(mtr_ctx *ctx, const ConsArgs &a, const ConsWeights *qual, int bucket, unsigned n_tasks, unsigned longest)
{
    if (n_tasks == 0) return MTR_OK;
    const int64_t words = ((int64_t)(longest >> 4) + 1) * CPL * 64;
    const int64_t cap_words = (int64_t)(std::min(ctx->sw.scratch_max_gb, 0.25) * (double)(1ll << 30) / 4.0);      // a quarter of a GB at the most, under the context's scratch cap
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_tasks, (int64_t)ctx->n_cu * 16), cap_words / words));
    HIPCHK(ctx->d_co_dirs.ensure((size_t)(grid * words) * 4));
    if (qual) hipLaunchKernelGGL(mtr_k_cq_align<CPL>, dim3((unsigned)grid), dim3(64), 0, ctx->stream, ConsQArgs{ a, qual->win_qual, qual->qual_cap }, bucket, n_tasks, (uint32_t *)ctx->d_co_dirs, words);
    else hipLaunchKernelGGL(mtr_k_cons_align<CPL>, dim3((unsigned)grid), dim3(64), 0, ctx->stream, a, bucket, n_tasks, (uint32_t *)ctx->d_co_dirs, words);
    HIPCHK(hipGetLastError());
    return MTR_OK;
}

// the allele consensus, unweighted (qual == NULL) or quality-weighted: the checks, the lists and the alignments' schedule are one; the votes' table
// (BA_TAB or BAQ_TAB counters a position), the walk and the emission are the vote's own kernels
static mtr_status allele_consensus(mtr_ctx *ctx, const mtr_consensus_src *src, const ConsWeights *qual, int32_t band_extra, void *wait_stream,
                                   const mtr_consensus_dst *dst, int64_t *out_bases)
{
    if (!ctx || !out_bases) return MTR_ERR_BAD_ARG;
    *out_bases = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (!src) { ctx->err = "src is NULL"; return MTR_ERR_BAD_ARG; }
    const int64_t R = src->n_rows, S = src->n_support, NB = src->n_bases; const int32_t n_loci = src->n_loci;
    if (n_loci < 1 || n_loci > (1 << 30) - 1) { ctx->err = "n_loci = " + std::to_string(n_loci) + " outside 1..2^30 - 1"; return MTR_ERR_BAD_ARG; }
    if (R < 0 || R > (int64_t)INT32_MAX) { ctx->err = "n_rows = " + std::to_string(R) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (S < 0 || S > (int64_t)INT32_MAX) { ctx->err = "n_support = " + std::to_string(S) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (NB < 0 || NB > (int64_t)INT32_MAX) { ctx->err = "n_bases = " + std::to_string(NB) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (band_extra < 0 || band_extra > MTR_CONS_MAX_EXTRA) { ctx->err = "band_extra = " + std::to_string(band_extra) + " outside 0.." + std::to_string(MTR_CONS_MAX_EXTRA); return MTR_ERR_BAD_ARG; }
    if (qual && (qual->qual_cap < 1 || qual->qual_cap > MTR_CONSQ_MAX_CAP)) { ctx->err = "qual_cap = " + std::to_string(qual->qual_cap) + " outside 1.." + std::to_string(MTR_CONSQ_MAX_CAP); return MTR_ERR_BAD_ARG; }
    if (qual && S * qual->qual_cap >= (1ll << 31)) {
        ctx->err = "n_support " + std::to_string(S) + " x qual_cap " + std::to_string(qual->qual_cap) + " reaches 2^31: the weight sums are int32"; return MTR_ERR_BAD_ARG;
    }
    if (!src->win_off || !src->support_off || !src->zygosity || (R > 0 && (!src->row_read || !src->row_locus)) || (NB > 0 && (!src->win_bases || (qual && !qual->win_qual))) ||
        (S > 0 && (!src->read || !src->allele))) { ctx->err = "an input column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    {
        const DeviceCol cols[9] = {
            { src->row_read, R * 4, "src->row_read" }, { src->row_locus, R * 4, "src->row_locus" }, { src->win_off, (R + 1) * 8, "src->win_off" }, { src->win_bases, NB, "src->win_bases" },
            { qual ? qual->win_qual : nullptr, qual ? NB : 0, "win_qual" },
            { src->support_off, ((int64_t)n_loci + 1) * 8, "src->support_off" }, { src->read, S * 4, "src->read" }, { src->allele, S, "src->allele" }, { src->zygosity, n_loci, "src->zygosity" } };
        { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    }
    read_switches(ctx->sw);
    const size_t G = 2 * (size_t)n_loci, ns = (size_t)S;
    HIPCHK(ctx->d_co_i32.ensure((ns + 9 * G) * 4)); HIPCHK(ctx->d_co_i64.ensure(2 * (G + 1) * 8)); HIPCHK(ctx->d_co_tasks.ensure(std::max<size_t>(2 * ns, 1) * sizeof(int4)));
    { mtr_status st = columns_begin(ctx, wait_stream, ctx->d_co_state, CO_BAD, CO_STATE * 8); if (st != MTR_OK) return st; }
    ConsArgs a{};
    a.row_read = src->row_read; a.row_locus = src->row_locus; a.R = R; a.win_off = src->win_off; a.win_bases = src->win_bases; a.n_bases = NB;
    a.support_off = src->support_off; a.sup_read = src->read; a.sup_allele = src->allele; a.zygosity = src->zygosity; a.S = S; a.n_loci = n_loci; a.band_extra = band_extra;
    int32_t *i32 = ctx->d_co_i32;
    a.ent_row = i32; a.bb_ent = i32 + ns; a.bb_row = a.bb_ent + G; a.bb_read = a.bb_row + G; a.bb_len = a.bb_read + G; a.members = a.bb_len + G; a.aligned = a.members + G;
    a.skipped = a.aligned + G; a.tab_len = a.skipped + G; a.cons_len = a.tab_len + G;
    a.tab_off = ctx->d_co_i64; a.cons_off = a.tab_off + G + 1; a.tasks = ctx->d_co_tasks;
    a.bad = ctx->d_co_state; a.state = (unsigned *)(a.bad + CO_BAD);
    const auto blocks = [](int64_t n) { return dim3((unsigned)((std::max<int64_t>(n, 1) + CO_BLOCK - 1) / CO_BLOCK)); };
    const dim3 blk(CO_BLOCK);
    unsigned long long bad[CO_BAD];
    hipLaunchKernelGGL(mtr_k_cons_check, blocks(std::max<int64_t>(R, n_loci)), blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, bad, a.bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0] != ~0ull) { ctx->err = "row " + std::to_string(bad[0]) + " is out of order: the rows must ascend by (read, locus), each pair once, none negative"; return MTR_ERR_BAD_ARG; }
    if (bad[1] != ~0ull) { ctx->err = "win_off at row " + std::to_string(bad[1]) + " does not ascend from 0 to n_bases, or the window is above 2^30 bases"; return MTR_ERR_BAD_ARG; }
    if (bad[2] != ~0ull) { ctx->err = "locus " + std::to_string(bad[2]) + ": support_off does not ascend from 0 to n_support, or the zygosity is above 2"; return MTR_ERR_BAD_ARG; }
    if (S > 0) {
        hipLaunchKernelGGL(mtr_k_cons_members, blocks(S), blk, 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_sync(ctx, bad, a.bad, sizeof bad, hipMemcpyDeviceToHost));
        if (bad[3] != ~0ull) {
            int32_t rd = 0;
            HIPCHK(copy_sync(ctx, &rd, src->read + bad[3], 4, hipMemcpyDeviceToHost));
            ctx->err = "support entry " + std::to_string(bad[3]) + " (read " + std::to_string(rd) + ") has no row of its (read, locus)";
            return MTR_ERR_BAD_ARG;
        }
        if (bad[4] != ~0ull) { ctx->err = "support entry " + std::to_string(bad[4]) + ": the allele column is not 0 .. 0 1 .. 1 within its locus"; return MTR_ERR_BAD_ARG; }
    }
    HIPCHK(hipMemsetAsync(a.aligned, 0, 2 * G * 4, ctx->stream));                                      // aligned | skipped
    hipLaunchKernelGGL(mtr_k_cons_alleles, blocks((int64_t)G), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)a.tab_len, (int64_t)G, a.tab_off);
    if (S > 0) hipLaunchKernelGGL(mtr_k_cons_tasks, blocks(S), blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    unsigned state[CO_STATE]; int64_t tab_positions = 0;
    HIPCHK(hipMemcpyAsync(&tab_positions, a.tab_off + G, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(copy_sync(ctx, state, a.state, sizeof state, hipMemcpyDeviceToHost));
    if (tab_positions < 0 || (int64_t)state[0] + state[1] > S || state[2] > 2 * BA_MAX_WINDOW || state[3] > 2 * BA_MAX_WINDOW) { ctx->err = "the consensus' task lists failed on the device"; return MTR_ERR_HIP; }
    const size_t tab_ints = (size_t)tab_positions * (qual ? BAQ_TAB : BA_TAB);
    HIPCHK(ctx->d_co_tab.ensure(std::max<size_t>(tab_ints, 1) * 4));
    a.tab = ctx->d_co_tab;
    if (tab_positions > 0) HIPCHK(hipMemsetAsync(a.tab, 0, tab_ints * 4, ctx->stream));
    { mtr_status st = cons_align_bucket<1>(ctx, a, qual, 0, state[0], state[2]); if (st != MTR_OK) return st; }
    { mtr_status st = cons_align_bucket<2>(ctx, a, qual, 1, state[1], state[3]); if (st != MTR_OK) return st; }
    const dim3 per_allele((unsigned)std::min<int64_t>((int64_t)G, CO_MAX_GRID));
    if (qual) hipLaunchKernelGGL(mtr_k_cq_emit<0>, per_allele, blk, 0, ctx->stream, ConsQArgs{ a, qual->win_qual, qual->qual_cap });
    else hipLaunchKernelGGL(mtr_k_cons_emit<0>, per_allele, blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)a.cons_len, (int64_t)G, a.cons_off);
    HIPCHK(hipGetLastError());
    int64_t T = 0;
    HIPCHK(copy_sync(ctx, &T, a.cons_off + G, 8, hipMemcpyDeviceToHost));
    if (T < 0) { ctx->err = "the consensus' emission lengths failed on the device"; return MTR_ERR_HIP; }
    *out_bases = T;
    if (!dst) return MTR_OK;
    if (dst->cap_alleles < (int64_t)G) { ctx->err = "destination holds " + std::to_string(dst->cap_alleles) + " alleles, " + std::to_string(G) + " needed"; return MTR_ERR_OVERFLOW; }
    if (dst->cap_bases < T) { ctx->err = "destination holds " + std::to_string(dst->cap_bases) + " bases, " + std::to_string(T) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->cons_off || !dst->backbone_read || !dst->backbone_len || !dst->members || !dst->aligned || !dst->skipped || (T > 0 && (!dst->bases || !dst->votes))) {
        ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG;
    }
    a.bases = dst->bases; a.votes = dst->votes;
    if (T > 0) {
        if (qual) hipLaunchKernelGGL(mtr_k_cq_emit<1>, per_allele, blk, 0, ctx->stream, ConsQArgs{ a, qual->win_qual, qual->qual_cap });
        else hipLaunchKernelGGL(mtr_k_cons_emit<1>, per_allele, blk, 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(dst->cons_off, a.cons_off, (G + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    const struct { int32_t *to; const int32_t *from; } cols[5] = { { dst->backbone_read, a.bb_read }, { dst->backbone_len, a.bb_len }, { dst->members, a.members }, { dst->aligned, a.aligned },
                                                                   { dst->skipped, a.skipped } };
    for (const auto &c : cols) HIPCHK(hipMemcpyAsync(c.to, c.from, G * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

extern "C" mtr_status mtr_allele_consensus_device(mtr_ctx *ctx, const mtr_consensus_src *src, int32_t band_extra, void *wait_stream,
                                                  const mtr_consensus_dst *dst, int64_t *out_bases)
{
    return allele_consensus(ctx, src, nullptr, band_extra, wait_stream, dst, out_bases);
}
extern "C" mtr_status mtr_allele_consensus_quality_device(mtr_ctx *ctx, const mtr_consensus_src *src, const uint8_t *win_qual, int32_t band_extra, int32_t qual_cap,
                                                          void *wait_stream, const mtr_consensus_dst *dst, int64_t *out_bases)
{
    const ConsWeights qual = { win_qual, qual_cap };
    return allele_consensus(ctx, src, &qual, band_extra, wait_stream, dst, out_bases);
}

// ---- the motif structure of windows (window_structure.hip.inc) ---------------------------------------------------------------------------
template <int UB, bool WIDE>
static void ws_launch_bin(mtr_ctx *ctx, const WsArgs &a, unsigned first, unsigned n_tasks)
{
    if (n_tasks > 0) hipLaunchKernelGGL((mtr_k_ws_lanes<UB, WIDE>), dim3((n_tasks + 63) / 64), dim3(64), 0, ctx->stream, a, first, n_tasks);
}

// The device's checks of the windows' columns, for the window structure and the window edits alike: the check and the base kernels on the call's
// state (a.bad = WS_BAD words at ~0 | the keys' counts, zeroed), one look at it, the smallest offender of each kind refused in the one set of
// words, and the keys' counts for the caller's bins.
struct WsCounts { unsigned long long bad[WS_BAD]; unsigned count[WS_KEYS]; };
static_assert(sizeof(WsCounts) == WS_BAD * 8 + WS_KEYS * 4, "the state's layout");
static mtr_status ws_device_checks(mtr_ctx *ctx, const WsArgs &a, size_t nw, WsCounts &st)
{
    const dim3 per_window((unsigned)((nw + WS_BLOCK - 1) / WS_BLOCK)), blk(WS_BLOCK);
    hipLaunchKernelGGL(mtr_k_ws_check, per_window, blk, 0, ctx->stream, a);
    if (a.n_bases > 0) {
        const int64_t words = (((int64_t)((uintptr_t)a.win_bases & 7) + a.n_bases - 1) >> 3) + 1;
        hipLaunchKernelGGL(mtr_k_ws_bases, dim3((unsigned)std::min<int64_t>((words + WS_BLOCK - 1) / WS_BLOCK, 1 << 16)), blk, 0, ctx->stream, a.win_bases, a.n_bases, words, a.bad);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, &st, a.bad, sizeof st, hipMemcpyDeviceToHost));
    if (st.bad[0] != ~0ull) { ctx->err = "win_off at window " + std::to_string(st.bad[0]) + " does not ascend from 0 to n_bases"; return MTR_ERR_BAD_ARG; }
    if (st.bad[1] != ~0ull) {
        int32_t k = 0;
        HIPCHK(copy_sync(ctx, &k, a.win_struct + st.bad[1], 4, hipMemcpyDeviceToHost));
        ctx->err = "window " + std::to_string(st.bad[1]) + ": win_struct " + std::to_string(k) + " outside 0.." + std::to_string(a.n_structs - 1); return MTR_ERR_BAD_ARG;
    }
    if (st.bad[2] != ~0ull) {
        uint8_t c = 0;
        HIPCHK(copy_sync(ctx, &c, a.win_bases + st.bad[2], 1, hipMemcpyDeviceToHost));
        ctx->err = "win_bases at " + std::to_string(st.bad[2]) + ": code " + std::to_string((int)c) + " is above 3"; return MTR_ERR_BAD_ARG;
    }
    return MTR_OK;
}

extern "C" mtr_status mtr_window_structure_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, const int32_t *struct_off, int32_t n_structs,
                                                  const int64_t *win_off, const uint8_t *win_bases, const int32_t *win_struct, int64_t n_windows, int64_t n_bases,
                                                  int32_t gain, int32_t mismatch, int32_t indel, void *wait_stream, const mtr_window_structure_dst *dst)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    const int64_t N = n_windows;
    const bool columns_null = !win_off || (N > 0 && !win_struct) || (n_bases > 0 && !win_bases) || !dst || (N > 0 && (!dst->seg || !dst->score || !dst->ratio || !dst->skipped));
    if (!wsa_check(motifs, motif_off, struct_off, n_structs, columns_null, N, n_bases, gain, mismatch, indel, ctx->err)) return MTR_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    const DeviceCol cols[3] = { { win_off, (N + 1) * 8, "win_off" }, { win_bases, n_bases, "win_bases" }, { win_struct, N * 4, "win_struct" } };
    { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    std::vector<WsStruct> structs((size_t)n_structs);
    for (int32_t k = 0; k < n_structs; k++) structs[(size_t)k] = wsa_struct(motifs, motif_off, struct_off, k);
    const size_t nw = std::max<size_t>((size_t)N, 1);
    HIPCHK(ctx->d_ws_structs.ensure(structs.size() * sizeof(WsStruct))); HIPCHK(ctx->d_ws_i32.ensure(2 * nw * 4)); HIPCHK(ctx->d_ws_raw.ensure(nw * sizeof(WsRaw)));
    { mtr_status st = columns_begin(ctx, wait_stream, ctx->d_ws_state, WS_BAD, 2 * WS_KEYS * 4); if (st != MTR_OK) return st; }
    HIPCHK(copy_sync(ctx, ctx->d_ws_structs, structs.data(), structs.size() * sizeof(WsStruct), hipMemcpyHostToDevice));
    WsArgs a{};
    a.win_off = win_off; a.win_bases = win_bases; a.win_struct = win_struct; a.N = N; a.n_bases = n_bases; a.n_structs = n_structs; a.structs = ctx->d_ws_structs;
    a.bad = ctx->d_ws_state; a.count = (unsigned *)(a.bad + WS_BAD); a.cursor = a.count + WS_KEYS;
    a.key = ctx->d_ws_i32; a.tasks = a.key + nw; a.raw = ctx->d_ws_raw; a.G = gain; a.MM = mismatch; a.D = indel;
    const dim3 per_window((unsigned)((nw + WS_BLOCK - 1) / WS_BLOCK)), blk(WS_BLOCK);
    WsCounts st;
    { mtr_status rc = ws_device_checks(ctx, a, nw, st); if (rc != MTR_OK) return rc; }
    if (dst->cap_windows < N) { ctx->err = "destination holds " + std::to_string(dst->cap_windows) + " windows, " + std::to_string(N) + " needed"; return MTR_ERR_OVERFLOW; }
    if (N == 0) return MTR_OK;
    unsigned bin_first[WS_BINS + 1] = { 0 };
    for (int b = 0; b < WS_BINS; b++) { unsigned n = 0; for (int k = 0; k < WS_CLASSES; k++) n += st.count[b * WS_CLASSES + k]; bin_first[b + 1] = bin_first[b] + n; }
    if ((int64_t)bin_first[WS_BINS] > N) { ctx->err = "the window structure's task counts failed on the device"; return MTR_ERR_HIP; }
    hipLaunchKernelGGL(mtr_k_ws_tasks, per_window, blk, 0, ctx->stream, a);
    ws_launch_bin<8, false>(ctx, a, bin_first[0], bin_first[1] - bin_first[0]);
    ws_launch_bin<16, false>(ctx, a, bin_first[1], bin_first[2] - bin_first[1]);
    ws_launch_bin<32, false>(ctx, a, bin_first[2], bin_first[3] - bin_first[2]);
    ws_launch_bin<8, true>(ctx, a, bin_first[3], bin_first[4] - bin_first[3]);
    ws_launch_bin<16, true>(ctx, a, bin_first[4], bin_first[5] - bin_first[4]);
    a.seg = dst->seg; a.score = dst->score; a.ratio = dst->ratio; a.skipped = dst->skipped;
    hipLaunchKernelGGL(mtr_k_ws_output, per_window, blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- the edits of windows (window_edits.hip.inc) -----------------------------------------------------------------------------------------
// The window structure's checks and task list on buffers of this call's own, then the groups' rows, one look at them, and the rounds: the groups
// in task order whatever their bins, their slots side by side, as many as the transient cap holds (one at the least): the usual call is ONE round.
// Count: per round the rows, then the walk that counts.  The offset
// scan, one look at the total.  Emit: per round the walk that writes - after the rows once more when there was more than one round, since a
// round's decisions are gone when the next has run.
struct WeRound { int bin; unsigned g_first, groups; int round; };

template <int UB, bool WIDE>
static void we_launch_rows(mtr_ctx *ctx, const WeArgs &a, const WeRound &r)
{
    hipLaunchKernelGGL((mtr_k_we_rows<UB, WIDE>), dim3(r.groups), dim3(64), 0, ctx->stream, a, r.g_first);
}
static void we_rows_of(mtr_ctx *ctx, const WeArgs &a, const WeRound &r)
{
    switch (r.bin) {
        case 0: we_launch_rows<8, false>(ctx, a, r); break;
        case 1: we_launch_rows<16, false>(ctx, a, r); break;
        case 2: we_launch_rows<32, false>(ctx, a, r); break;
        case 3: we_launch_rows<8, true>(ctx, a, r); break;
        default: we_launch_rows<16, true>(ctx, a, r); break;
    }
}

extern "C" mtr_status mtr_window_edits_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, const int32_t *struct_off, int32_t n_structs,
                                              const int64_t *win_off, const uint8_t *win_bases, const int32_t *win_struct, int64_t n_windows, int64_t n_bases,
                                              int32_t gain, int32_t mismatch, int32_t indel, void *wait_stream, int64_t *out_edits)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    ctx->we_ready = false;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    const int64_t N = n_windows;
    const bool columns_null = !win_off || (N > 0 && !win_struct) || (n_bases > 0 && !win_bases) || !out_edits;
    if (!wsa_check(motifs, motif_off, struct_off, n_structs, columns_null, N, n_bases, gain, mismatch, indel, ctx->err)) return MTR_ERR_BAD_ARG;
    *out_edits = 0;
    HIPCHK(hipSetDevice(ctx->device));
    const DeviceCol cols[3] = { { win_off, (N + 1) * 8, "win_off" }, { win_bases, n_bases, "win_bases" }, { win_struct, N * 4, "win_struct" } };
    { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    std::vector<WsStruct> structs((size_t)n_structs);
    for (int32_t k = 0; k < n_structs; k++) structs[(size_t)k] = wsa_struct(motifs, motif_off, struct_off, k);
    const size_t nw = std::max<size_t>((size_t)N, 1), max_groups = nw / 64 + WS_BINS;
    HIPCHK(ctx->d_we_structs.ensure(structs.size() * sizeof(WsStruct))); HIPCHK(ctx->d_we_i32.ensure((4 * nw + max_groups) * 4)); HIPCHK(ctx->d_we_raw.ensure(nw * sizeof(WsRaw)));
    HIPCHK(ctx->d_we_cnt.ensure(nw * sizeof(WeCount))); HIPCHK(ctx->d_we_i64.ensure(max_groups * 8)); HIPCHK(ctx->d_we_off.ensure((nw + 1) * 8));
    HIPCHK(ctx->d_we_seg.ensure(nw * 4 * WS_MAX_SEGMENTS * 4)); HIPCHK(ctx->d_we_score.ensure(nw * 4)); HIPCHK(ctx->d_we_skipped.ensure(nw));
    { mtr_status st = columns_begin(ctx, wait_stream, ctx->d_we_state, WS_BAD, 2 * WS_KEYS * 4 + 8); if (st != MTR_OK) return st; }
    HIPCHK(copy_sync(ctx, ctx->d_we_structs, structs.data(), structs.size() * sizeof(WsStruct), hipMemcpyHostToDevice));
    WeArgs a{};
    WsArgs &w = a.ws;
    w.win_off = win_off; w.win_bases = win_bases; w.win_struct = win_struct; w.N = N; w.n_bases = n_bases; w.n_structs = n_structs; w.structs = ctx->d_we_structs;
    w.bad = ctx->d_we_state; w.count = (unsigned *)(w.bad + WS_BAD); w.cursor = w.count + WS_KEYS; a.differs = (unsigned long long *)(w.cursor + WS_KEYS);       // the window structure's state | differs
    HIPCHK(hipMemsetAsync(a.differs, 0xff, 8, ctx->stream));
    w.key = ctx->d_we_i32; w.tasks = w.key + nw; a.end_id = w.tasks + nw; a.n_edits = a.end_id + nw; a.grows = a.n_edits + nw;
    w.raw = ctx->d_we_raw; w.G = gain; w.MM = mismatch; w.D = indel;
    a.cnt = ctx->d_we_cnt; a.gslot = ctx->d_we_i64; a.off = ctx->d_we_off; a.seg = ctx->d_we_seg; a.score = ctx->d_we_score; a.skipped = ctx->d_we_skipped;
    const dim3 per_window((unsigned)((nw + WS_BLOCK - 1) / WS_BLOCK)), blk(WS_BLOCK);
    WsCounts st;
    { mtr_status rc = ws_device_checks(ctx, w, nw, st); if (rc != MTR_OK) return rc; }
    ctx->we_rounds = 0;
    if (N == 0) {
        HIPCHK(hipMemsetAsync(ctx->d_we_off, 0, 8, ctx->stream)); HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->we_ready = true; ctx->we_windows = 0; ctx->we_edits = 0;
        return MTR_OK;
    }
    unsigned groups = 0;
    for (int b = 0; b < WS_BINS; b++) {
        unsigned n = 0; for (int k = 0; k < WS_CLASSES; k++) n += st.count[b * WS_CLASSES + k];
        a.bin_first[b + 1] = a.bin_first[b] + n; a.grp_first[b] = groups; groups += (n + 63) / 64;
    }
    a.grp_first[WS_BINS] = groups;
    if ((int64_t)a.bin_first[WS_BINS] > N || groups > max_groups) { ctx->err = "the window edits' task counts failed on the device"; return MTR_ERR_HIP; }
    HIPCHK(hipMemsetAsync(a.n_edits, 0, nw * 4, ctx->stream));
    hipLaunchKernelGGL(mtr_k_ws_tasks, per_window, blk, 0, ctx->stream, w);
    std::vector<WeRound> parts;                                          // a round's groups of one bin; a round is the parts of one number
    int n_rounds = 0;
    size_t scratch_words = 1;
    if (groups > 0) {
        hipLaunchKernelGGL(mtr_k_we_groups, dim3(groups), dim3(64), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        std::vector<int32_t> grows((size_t)groups);
        HIPCHK(copy_sync(ctx, grows.data(), a.grows, (size_t)groups * 4, hipMemcpyDeviceToHost));
        const char *e = getenv("MTR_TEST_WE_SCRATCH_BYTES");
        const size_t cap_words = (size_t)std::max<long long>(e ? atoll(e) : (long long)MTR_WE_SCRATCH_BYTES, 4) / 4;
        static const int bin_ub[WS_BINS] = { 8, 16, 32, 8, 16 };
        std::vector<int64_t> gslot((size_t)groups);
        size_t used = 0;
        for (int b = 0; b < WS_BINS; b++)
            for (unsigned g = a.grp_first[b]; g < a.grp_first[b + 1]; g++) {
                if (grows[g] < 1 || grows[g] > WS_MAX_WINDOW + 1) { ctx->err = "the window edits' group rows failed on the device"; return MTR_ERR_HIP; }
                const size_t words = (size_t)grows[g] * (size_t)we_row_words(bin_ub[b]) * 64;
                if (g == 0 || used + words > cap_words) { n_rounds++; used = 0; }
                if (parts.empty() || parts.back().round != n_rounds - 1 || parts.back().bin != b) parts.push_back(WeRound{ b, g, 0, n_rounds - 1 });
                gslot[g] = (int64_t)used; used += words; parts.back().groups++;
                scratch_words = std::max(scratch_words, used);
            }
        HIPCHK(ctx->d_we_scratch.ensure(scratch_words * 4));
        HIPCHK(copy_sync(ctx, ctx->d_we_i64, gslot.data(), (size_t)groups * 8, hipMemcpyHostToDevice));
    }
    a.scratch = ctx->d_we_scratch;
    // a round's groups are consecutive whatever their bins: the rows one launch per part, either walk one launch per round
    const auto walk_round = [&](int round, bool rows, bool emit) {
        unsigned g0 = 0, ng = 0;
        for (const WeRound &r : parts) if (r.round == round) { if (ng == 0) g0 = r.g_first; ng += r.groups; if (rows) we_rows_of(ctx, a, r); }
        if (emit) hipLaunchKernelGGL(mtr_k_we_emit, dim3(ng), dim3(64), 0, ctx->stream, a, g0);
        else hipLaunchKernelGGL(mtr_k_we_count, dim3(ng), dim3(64), 0, ctx->stream, a, g0);
    };
    for (int k = 0; k < n_rounds; k++) walk_round(k, true, false);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)a.n_edits, N, ctx->d_we_off.p);
    HIPCHK(hipGetLastError());
    int64_t T = 0; unsigned long long differs = ~0ull;
    HIPCHK(hipMemcpyAsync(&T, ctx->d_we_off + N, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(copy_sync(ctx, &differs, a.differs, 8, hipMemcpyDeviceToHost));
    if (differs != ~0ull) {
        WeCount k{}; WsRaw raw{}; int32_t end = 0;
        HIPCHK(copy_sync(ctx, &k, a.cnt + differs, sizeof k, hipMemcpyDeviceToHost)); HIPCHK(copy_sync(ctx, &raw, w.raw + differs, sizeof raw, hipMemcpyDeviceToHost));
        HIPCHK(copy_sync(ctx, &end, a.end_id + differs, 4, hipMemcpyDeviceToHost));
        char buf[256];
        snprintf(buf, sizeof buf, ": the stored decisions are not the path of its rows (end %d; entry, copies, matches walked %llx %llx %llx, carried %llx %llx %llx; %d edits, gave up %d)", end,
                 (unsigned long long)k.entry, (unsigned long long)k.copies, (unsigned long long)k.matches, (unsigned long long)raw.entry, (unsigned long long)raw.copies, (unsigned long long)raw.matches, k.edits, k.bad);
        ctx->err = "window " + std::to_string(differs) + buf; return MTR_ERR_HIP;
    }
    HIPCHK(ctx->d_we_edits.ensure((size_t)std::max<int64_t>(T, 1) * WE_FIELDS * 4));
    a.edits = ctx->d_we_edits;
    for (int k = 0; k < n_rounds; k++) walk_round(k, n_rounds > 1, true);
    hipLaunchKernelGGL(mtr_k_we_output, per_window, blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, &differs, a.differs, 8, hipMemcpyDeviceToHost));
    if (differs != ~0ull) { ctx->err = "window " + std::to_string(differs) + ": the walk that writes is not the walk that counted"; return MTR_ERR_HIP; }
    ctx->we_ready = true; ctx->we_windows = N; ctx->we_edits = T; ctx->we_rounds = n_rounds;
    *out_edits = T;
    return MTR_OK;
}

extern "C" mtr_status mtr_window_edits_copy_device(mtr_ctx *ctx, const mtr_window_edits_dst *dst)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (!ctx->we_ready) { ctx->err = "no edits kept: mtr_window_edits_device comes first"; return MTR_ERR_BAD_ARG; }
    if (!dst) { ctx->err = "dst is NULL"; return MTR_ERR_BAD_ARG; }
    const int64_t N = ctx->we_windows, T = ctx->we_edits;
    if (dst->cap_windows < N) { ctx->err = "destination holds " + std::to_string(dst->cap_windows) + " windows, " + std::to_string(N) + " needed"; return MTR_ERR_OVERFLOW; }
    if (dst->cap_edits < T) { ctx->err = "destination holds " + std::to_string(dst->cap_edits) + " edits, " + std::to_string(T) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->off || (T > 0 && !dst->edits) || (N > 0 && (!dst->seg || !dst->score || !dst->skipped))) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const DeviceCol cols[5] = { { dst->off, (N + 1) * 8, "dst->off" }, { dst->edits, T * WE_FIELDS * 4, "dst->edits" }, { dst->seg, N * 4 * WS_MAX_SEGMENTS * 4, "dst->seg" },
                                { dst->score, N * 4, "dst->score" }, { dst->skipped, N, "dst->skipped" } };
    { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    const void *from[5] = { ctx->d_we_off.p, ctx->d_we_edits.p, ctx->d_we_seg.p, ctx->d_we_score.p, ctx->d_we_skipped.p };
    for (int k = 0; k < 5; k++)
        if (cols[k].bytes > 0) HIPCHK(hipMemcpyAsync(const_cast<void *>(cols[k].p), from[k], (size_t)cols[k].bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- the sequence allele calls (seq_calls.hip.inc) -------------------------------------------------------------------------------------------
// The consensus' checks in its order, then the members' rows, the loci's pair counts and their scan, one look at P, the pairs' tasks, one look
// at the buckets' counts, the distances bucket by bucket, the split.  Everything lands in buffers of the context's own, kept for the copy.
static_assert(MTR_SEQ_MAX_DIST == SQ_MAX_DIST && MTR_SEQ_MAX_MEMBERS == SQ_MAX_MEMBERS, "the sequence calls' limits");
static_assert(sizeof(mtr_seq_params) == sizeof(SqParams), "the sequence calls' parameters");

template <int ROWS, int CPL>
static void seq_dist_bucket(mtr_ctx *ctx, const SeqArgs &a, const int4 *tasks, int64_t step, unsigned n_tasks)
{
    if (n_tasks == 0) return;
    const unsigned groups = (n_tasks + (unsigned)ROWS - 1u) / (unsigned)ROWS;
    hipLaunchKernelGGL((mtr_k_seq_dist<ROWS, CPL>), dim3(std::min<unsigned>(groups, SQ_MAX_GRID)), dim3(64), 0, ctx->stream, a, tasks, step, n_tasks);
}

extern "C" mtr_status mtr_call_alleles_sequence_device(mtr_ctx *ctx, const mtr_consensus_src *src, const int32_t *value, const mtr_seq_params *prm,
                                                       void *wait_stream, int64_t *out_support, int64_t *out_pairs)
{
    if (!ctx || !out_support || !out_pairs) return MTR_ERR_BAD_ARG;
    *out_support = 0; *out_pairs = 0;
    ctx->sq_ready = false;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (!src || !prm) { ctx->err = "src or prm is NULL"; return MTR_ERR_BAD_ARG; }
    const int64_t R = src->n_rows, S = src->n_support, NB = src->n_bases; const int32_t n_loci = src->n_loci;
    if (n_loci < 1 || n_loci > (1 << 30) - 1) { ctx->err = "n_loci = " + std::to_string(n_loci) + " outside 1..2^30 - 1"; return MTR_ERR_BAD_ARG; }
    if (R < 0 || R > (int64_t)INT32_MAX) { ctx->err = "n_rows = " + std::to_string(R) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (S < 0 || S > (int64_t)INT32_MAX) { ctx->err = "n_support = " + std::to_string(S) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (NB < 0 || NB > (int64_t)INT32_MAX) { ctx->err = "n_bases = " + std::to_string(NB) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (prm->max_dist < 0 || prm->max_dist > MTR_SEQ_MAX_DIST) { ctx->err = "max_dist = " + std::to_string(prm->max_dist) + " outside 0.." + std::to_string(MTR_SEQ_MAX_DIST); return MTR_ERR_BAD_ARG; }
    if (prm->min_support < 1) { ctx->err = "min_support " + std::to_string(prm->min_support) + ": at least 1"; return MTR_ERR_BAD_ARG; }
    if (prm->min_percent < 0 || prm->min_percent > 50) { ctx->err = "min_percent " + std::to_string(prm->min_percent) + " outside 0..50"; return MTR_ERR_BAD_ARG; }
    if (prm->min_sep < 1) { ctx->err = "min_sep " + std::to_string(prm->min_sep) + ": at least 1"; return MTR_ERR_BAD_ARG; }
    if (prm->min_gain < 0 || prm->min_gain > 100) { ctx->err = "min_gain " + std::to_string(prm->min_gain) + " outside 0..100"; return MTR_ERR_BAD_ARG; }
    if (!src->win_off || !src->support_off || (R > 0 && (!src->row_read || !src->row_locus)) || (NB > 0 && !src->win_bases) || (S > 0 && (!src->read || !value))) {
        ctx->err = "an input column is NULL"; return MTR_ERR_BAD_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    {
        const DeviceCol cols[7] = {
            { src->row_read, R * 4, "src->row_read" }, { src->row_locus, R * 4, "src->row_locus" }, { src->win_off, (R + 1) * 8, "src->win_off" }, { src->win_bases, NB, "src->win_bases" },
            { src->support_off, ((int64_t)n_loci + 1) * 8, "src->support_off" }, { src->read, S * 4, "src->read" }, { value, S * 4, "value" } };
        { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    }
    const size_t nl = (size_t)n_loci, ns = std::max<size_t>((size_t)S, 1);
    HIPCHK(ctx->d_sq_i32.ensure((ns + nl) * 4)); HIPCHK(ctx->d_sq_pair_off.ensure((nl + 1) * 8)); HIPCHK(ctx->d_sq_off.ensure((nl + 1) * 8));
    HIPCHK(ctx->d_sq_value.ensure(ns * 4)); HIPCHK(ctx->d_sq_read.ensure(ns * 4)); HIPCHK(ctx->d_sq_dtm.ensure(ns * 4)); HIPCHK(ctx->d_sq_allele.ensure(ns));
    HIPCHK(ctx->d_sq_zyg.ensure(nl)); HIPCHK(ctx->d_sq_skipped.ensure(nl)); HIPCHK(ctx->d_sq_call.ensure(2 * nl * 4)); HIPCHK(ctx->d_sq_sup.ensure(2 * nl * 4));
    HIPCHK(ctx->d_sq_medoid.ensure(2 * nl * 4)); HIPCHK(ctx->d_sq_cost.ensure(2 * nl * 8));
    { mtr_status st = columns_begin(ctx, wait_stream, ctx->d_sq_state, CO_BAD, SQ_STATE * 4); if (st != MTR_OK) return st; }
    SeqArgs a{};
    ConsArgs &c = a.c;
    c.row_read = src->row_read; c.row_locus = src->row_locus; c.R = R; c.win_off = src->win_off; c.win_bases = src->win_bases; c.n_bases = NB;
    c.support_off = src->support_off; c.sup_read = src->read; c.S = S; c.n_loci = n_loci;
    c.ent_row = ctx->d_sq_i32; c.bad = ctx->d_sq_state; c.state = (unsigned *)(c.bad + CO_BAD);
    a.value = value; a.prm = { prm->max_dist, prm->min_support, prm->min_percent, prm->min_sep, prm->min_gain };
    a.npairs = ctx->d_sq_i32 + ns; a.pair_off = ctx->d_sq_pair_off;
    a.o_value = ctx->d_sq_value; a.o_read = ctx->d_sq_read; a.o_dtm = ctx->d_sq_dtm; a.o_allele = ctx->d_sq_allele; a.o_zyg = ctx->d_sq_zyg; a.o_skipped = ctx->d_sq_skipped;
    a.o_call = ctx->d_sq_call; a.o_sup = ctx->d_sq_sup; a.o_medoid = ctx->d_sq_medoid; a.o_cost = ctx->d_sq_cost;
    const auto blocks = [](int64_t n) { return dim3((unsigned)((std::max<int64_t>(n, 1) + SQ_BLOCK - 1) / SQ_BLOCK)); };
    const dim3 blk(SQ_BLOCK);
    unsigned long long bad[CO_BAD];
    hipLaunchKernelGGL(mtr_k_seq_check, blocks(std::max<int64_t>(R, n_loci)), blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, bad, c.bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0] != ~0ull) { ctx->err = "row " + std::to_string(bad[0]) + " is out of order: the rows must ascend by (read, locus), each pair once, none negative"; return MTR_ERR_BAD_ARG; }
    if (bad[1] != ~0ull) { ctx->err = "win_off at row " + std::to_string(bad[1]) + " does not ascend from 0 to n_bases, or the window is above 2^30 bases"; return MTR_ERR_BAD_ARG; }
    if (bad[2] != ~0ull) { ctx->err = "locus " + std::to_string(bad[2]) + ": support_off does not ascend from 0 to n_support"; return MTR_ERR_BAD_ARG; }
    if (S > 0) {
        hipLaunchKernelGGL(mtr_k_seq_members, blocks(S), blk, 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_sync(ctx, bad, c.bad, sizeof bad, hipMemcpyDeviceToHost));
        if (bad[3] != ~0ull) {
            int32_t rd = 0;
            HIPCHK(copy_sync(ctx, &rd, src->read + bad[3], 4, hipMemcpyDeviceToHost));
            ctx->err = "support entry " + std::to_string(bad[3]) + " (read " + std::to_string(rd) + ") has no row of its (read, locus)";
            return MTR_ERR_BAD_ARG;
        }
    }
    hipLaunchKernelGGL(mtr_k_seq_loci, blocks(n_loci), blk, 0, ctx->stream, a);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)a.npairs, (int64_t)n_loci, a.pair_off);
    HIPCHK(hipGetLastError());
    int64_t P = 0;
    HIPCHK(copy_sync(ctx, &P, a.pair_off + n_loci, 8, hipMemcpyDeviceToHost));
    if (P < 0 || P > S * (SQ_MAX_MEMBERS - 1) / 2) { ctx->err = "the sequence calls' pair counts failed on the device"; return MTR_ERR_HIP; }
    if (P > (int64_t)INT32_MAX) { ctx->err = std::to_string(P) + " pairs are more than 2^31 - 1"; return MTR_ERR_OVERFLOW; }
    a.P = P;
    HIPCHK(ctx->d_sq_dist.ensure(std::max<size_t>((size_t)P, 1))); HIPCHK(ctx->d_sq_tasks.ensure(std::max<size_t>(2 * (size_t)P, 1) * sizeof(int4)));
    a.dist = ctx->d_sq_dist; a.tasks = ctx->d_sq_tasks;
    if (P > 0) {
        hipLaunchKernelGGL(mtr_k_seq_tasks, dim3((unsigned)std::min<int64_t>((P + SQ_BLOCK - 1) / SQ_BLOCK, SQ_MAX_GRID)), blk, 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        unsigned n[SQ_STATE];
        HIPCHK(copy_sync(ctx, n, c.state, sizeof n, hipMemcpyDeviceToHost));
        if ((int64_t)n[0] + n[1] > P || (int64_t)n[2] + n[3] > P) { ctx->err = "the sequence calls' task lists failed on the device"; return MTR_ERR_HIP; }
        const char *e = getenv("MTR_TEST_SEQ_ROWS");
        if (e && atoi(e) == 0) { seq_dist_bucket<1, 1>(ctx, a, a.tasks, 1, n[0]); seq_dist_bucket<1, 1>(ctx, a, a.tasks + P - 1, -1, n[1]); }
        else { seq_dist_bucket<4, 1>(ctx, a, a.tasks, 1, n[0]); seq_dist_bucket<2, 1>(ctx, a, a.tasks + P - 1, -1, n[1]); }
        seq_dist_bucket<1, 1>(ctx, a, a.tasks + P, 1, n[2]);
        seq_dist_bucket<1, 2>(ctx, a, a.tasks + 2 * P - 1, -1, n[3]);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mtr_k_seq_split, dim3((unsigned)std::min<int64_t>(n_loci, SQ_MAX_GRID)), dim3(64), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->d_sq_off, src->support_off, (nl + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->sq_ready = true; ctx->sq_loci = n_loci; ctx->sq_support = S; ctx->sq_pairs = P;
    *out_support = S; *out_pairs = P;
    return MTR_OK;
}

extern "C" mtr_status mtr_call_alleles_sequence_copy_device(mtr_ctx *ctx, const mtr_seq_calls_dst *dst)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (!ctx->sq_ready) { ctx->err = "no sequence calls kept: mtr_call_alleles_sequence_device comes first"; return MTR_ERR_BAD_ARG; }
    if (!dst) { ctx->err = "dst is NULL"; return MTR_ERR_BAD_ARG; }
    const int64_t L = ctx->sq_loci, S = ctx->sq_support, P = ctx->sq_pairs;
    if (dst->cap_loci < L) { ctx->err = "destination holds " + std::to_string(dst->cap_loci) + " loci, " + std::to_string(L) + " needed"; return MTR_ERR_OVERFLOW; }
    if (dst->cap_support < S) { ctx->err = "destination holds " + std::to_string(dst->cap_support) + " supporting rows, " + std::to_string(S) + " needed"; return MTR_ERR_OVERFLOW; }
    if (dst->cap_pairs < P) { ctx->err = "destination holds " + std::to_string(dst->cap_pairs) + " pairs, " + std::to_string(P) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->support_off || !dst->zygosity || !dst->call || !dst->call_support || !dst->medoid || !dst->cost || !dst->skipped || !dst->pair_off ||
        (S > 0 && (!dst->value || !dst->read || !dst->allele || !dst->dist_to_medoid)) || (P > 0 && !dst->dist)) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const DeviceCol cols[13] = { { dst->support_off, (L + 1) * 8, "dst->support_off" }, { dst->value, S * 4, "dst->value" }, { dst->read, S * 4, "dst->read" }, { dst->allele, S, "dst->allele" },
                                 { dst->dist_to_medoid, S * 4, "dst->dist_to_medoid" }, { dst->zygosity, L, "dst->zygosity" }, { dst->call, L * 8, "dst->call" },
                                 { dst->call_support, L * 8, "dst->call_support" }, { dst->medoid, L * 8, "dst->medoid" }, { dst->cost, L * 16, "dst->cost" }, { dst->skipped, L, "dst->skipped" },
                                 { dst->pair_off, (L + 1) * 8, "dst->pair_off" }, { dst->dist, P, "dst->dist" } };
    { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    const void *from[13] = { ctx->d_sq_off.p, ctx->d_sq_value.p, ctx->d_sq_read.p, ctx->d_sq_allele.p, ctx->d_sq_dtm.p, ctx->d_sq_zyg.p, ctx->d_sq_call.p, ctx->d_sq_sup.p, ctx->d_sq_medoid.p,
                             ctx->d_sq_cost.p, ctx->d_sq_skipped.p, ctx->d_sq_pair_off.p, ctx->d_sq_dist.p };
    for (int k = 0; k < 13; k++)
        if (cols[k].bytes > 0) HIPCHK(hipMemcpyAsync(const_cast<void *>(cols[k].p), from[k], (size_t)cols[k].bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- the genotype quality (genotype_quality.hip.inc) -----------------------------------------------------------------------------------------------
// The consensus' checks in its order with its own list kernels, cons_off on the device, then the destination - every refusal comes before the
// first kernel that is given dst -, the tasks, one look at the buckets' counts, the scores bucket by bucket, the loci.  Nothing is kept.
static_assert(sizeof(mtr_gq_params) == sizeof(GqParams), "the genotype quality's parameters");

template <int ROWS, int CPL>
static void gq_score_bucket(mtr_ctx *ctx, const GqArgs &a, const int4 *tasks, int64_t step, unsigned n_tasks)
{
    if (n_tasks == 0) return;
    const unsigned groups = (n_tasks + (unsigned)ROWS - 1u) / (unsigned)ROWS;
    hipLaunchKernelGGL((mtr_k_gq_score<ROWS, CPL>), dim3(std::min<unsigned>(groups, GQ_MAX_GRID)), dim3(64), 0, ctx->stream, a, tasks, step, n_tasks);
}

extern "C" mtr_status mtr_genotype_quality_device(mtr_ctx *ctx, const mtr_consensus_src *src, const uint8_t *win_qual, const int64_t *cons_off, const uint8_t *cons_bases,
                                                  int64_t n_cons, const mtr_gq_params *prm, void *wait_stream, const mtr_gq_dst *dst)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (!src || !prm || !dst) { ctx->err = "src, prm or dst is NULL"; return MTR_ERR_BAD_ARG; }
    const int64_t R = src->n_rows, S = src->n_support, NB = src->n_bases, NC = n_cons; const int32_t n_loci = src->n_loci;
    if (n_loci < 1 || n_loci > (1 << 30) - 1) { ctx->err = "n_loci = " + std::to_string(n_loci) + " outside 1..2^30 - 1"; return MTR_ERR_BAD_ARG; }
    if (R < 0 || R > (int64_t)INT32_MAX) { ctx->err = "n_rows = " + std::to_string(R) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (S < 0 || S > (int64_t)INT32_MAX) { ctx->err = "n_support = " + std::to_string(S) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (NB < 0 || NB > (int64_t)INT32_MAX) { ctx->err = "n_bases = " + std::to_string(NB) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (NC < 0 || NC > (int64_t)INT32_MAX) { ctx->err = "n_cons = " + std::to_string(NC) + " outside 0..2^31 - 1"; return MTR_ERR_BAD_ARG; }
    if (prm->band_extra < 0 || prm->band_extra > MTR_CONS_MAX_EXTRA) { ctx->err = "band_extra = " + std::to_string(prm->band_extra) + " outside 0.." + std::to_string(MTR_CONS_MAX_EXTRA); return MTR_ERR_BAD_ARG; }
    if (prm->qual_cap < 1 || prm->qual_cap > MTR_CONSQ_MAX_CAP) { ctx->err = "qual_cap = " + std::to_string(prm->qual_cap) + " outside 1.." + std::to_string(MTR_CONSQ_MAX_CAP); return MTR_ERR_BAD_ARG; }
    if (prm->gap_cap < 1 || prm->gap_cap > prm->qual_cap) { ctx->err = "gap_cap = " + std::to_string(prm->gap_cap) + " outside 1..qual_cap = " + std::to_string(prm->qual_cap); return MTR_ERR_BAD_ARG; }
    if (prm->read_cap < 1 || prm->read_cap > MTR_GQ_MAX_READ_CAP) { ctx->err = "read_cap = " + std::to_string(prm->read_cap) + " outside 1.." + std::to_string(MTR_GQ_MAX_READ_CAP); return MTR_ERR_BAD_ARG; }
    if (!src->win_off || !src->support_off || !src->zygosity || !cons_off || (R > 0 && (!src->row_read || !src->row_locus)) || (NB > 0 && !src->win_bases) || (NC > 0 && !cons_bases) ||
        (S > 0 && (!src->read || !src->allele))) { ctx->err = "an input column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t G = 2 * (int64_t)n_loci;
    {
        const DeviceCol cols[11] = {
            { src->row_read, R * 4, "src->row_read" }, { src->row_locus, R * 4, "src->row_locus" }, { src->win_off, (R + 1) * 8, "src->win_off" }, { src->win_bases, NB, "src->win_bases" },
            { win_qual, win_qual ? NB : 0, "win_qual" },
            { src->support_off, ((int64_t)n_loci + 1) * 8, "src->support_off" }, { src->read, S * 4, "src->read" }, { src->allele, S, "src->allele" }, { src->zygosity, n_loci, "src->zygosity" },
            { cons_off, (G + 1) * 8, "cons_off" }, { cons_bases, NC, "cons_bases" } };
        { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    }
    const size_t ns = std::max<size_t>((size_t)S, 1);
    HIPCHK(ctx->d_gq_i32.ensure(ns * 4)); HIPCHK(ctx->d_gq_tasks.ensure(4 * ns * sizeof(int4)));
    { mtr_status st = columns_begin(ctx, wait_stream, ctx->d_gq_state, CO_BAD, SQ_STATE * 4); if (st != MTR_OK) return st; }
    GqArgs a{};
    ConsArgs &c = a.c;
    c.row_read = src->row_read; c.row_locus = src->row_locus; c.R = R; c.win_off = src->win_off; c.win_bases = src->win_bases; c.n_bases = NB;
    c.support_off = src->support_off; c.sup_read = src->read; c.sup_allele = src->allele; c.zygosity = src->zygosity; c.S = S; c.n_loci = n_loci; c.band_extra = prm->band_extra;
    c.ent_row = ctx->d_gq_i32; c.bad = ctx->d_gq_state; c.state = (unsigned *)(c.bad + CO_BAD);
    a.win_qual = NB > 0 ? win_qual : nullptr; a.cons_off = cons_off; a.cons_bases = cons_bases; a.n_cons = NC;
    a.prm = { prm->band_extra, prm->qual_cap, prm->gap_cap, prm->read_cap };
    a.tasks = ctx->d_gq_tasks;
    const auto blocks = [](int64_t n) { return dim3((unsigned)((std::max<int64_t>(n, 1) + GQ_BLOCK - 1) / GQ_BLOCK)); };
    const dim3 blk(GQ_BLOCK);
    static_assert(GQ_BLOCK == CO_BLOCK, "the consensus' list kernels are launched with this block");
    unsigned long long bad[CO_BAD];
    hipLaunchKernelGGL(mtr_k_cons_check, blocks(std::max<int64_t>(R, n_loci)), blk, 0, ctx->stream, c);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, bad, c.bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0] != ~0ull) { ctx->err = "row " + std::to_string(bad[0]) + " is out of order: the rows must ascend by (read, locus), each pair once, none negative"; return MTR_ERR_BAD_ARG; }
    if (bad[1] != ~0ull) { ctx->err = "win_off at row " + std::to_string(bad[1]) + " does not ascend from 0 to n_bases, or the window is above 2^30 bases"; return MTR_ERR_BAD_ARG; }
    if (bad[2] != ~0ull) { ctx->err = "locus " + std::to_string(bad[2]) + ": support_off does not ascend from 0 to n_support, or the zygosity is above 2"; return MTR_ERR_BAD_ARG; }
    if (S > 0) hipLaunchKernelGGL(mtr_k_cons_members, blocks(S), blk, 0, ctx->stream, c);
    hipLaunchKernelGGL(mtr_k_gq_check, blocks(G), blk, 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, bad, c.bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[3] != ~0ull) {
        int32_t rd = 0;
        HIPCHK(copy_sync(ctx, &rd, src->read + bad[3], 4, hipMemcpyDeviceToHost));
        ctx->err = "support entry " + std::to_string(bad[3]) + " (read " + std::to_string(rd) + ") has no row of its (read, locus)";
        return MTR_ERR_BAD_ARG;
    }
    if (bad[4] != ~0ull) { ctx->err = "support entry " + std::to_string(bad[4]) + ": the allele column is not 0 .. 0 1 .. 1 within its locus"; return MTR_ERR_BAD_ARG; }
    if (bad[GQ_BAD_CONS] != ~0ull) {
        ctx->err = "allele " + std::to_string(bad[GQ_BAD_CONS]) + " (locus " + std::to_string(bad[GQ_BAD_CONS] >> 1) + "): cons_off does not ascend from 0 to n_cons"; return MTR_ERR_BAD_ARG;
    }
    if (dst->cap_support < S) { ctx->err = "destination holds " + std::to_string(dst->cap_support) + " supporting rows, " + std::to_string(S) + " needed"; return MTR_ERR_OVERFLOW; }
    if (dst->cap_loci < n_loci) { ctx->err = "destination holds " + std::to_string(dst->cap_loci) + " loci, " + std::to_string(n_loci) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->raw || !dst->pl || !dst->gt || !dst->gq || !dst->scored || !dst->unscored || (S > 0 && (!dst->score || !dst->best || !dst->margin))) {
        ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG;
    }
    {
        const int64_t L = n_loci;
        const DeviceCol cols[9] = { { dst->score, S * 8, "dst->score" }, { dst->best, S, "dst->best" }, { dst->margin, S * 4, "dst->margin" }, { dst->raw, L * 24, "dst->raw" },
                                    { dst->pl, L * 24, "dst->pl" }, { dst->gt, L, "dst->gt" }, { dst->gq, L * 8, "dst->gq" }, { dst->scored, L * 4, "dst->scored" },
                                    { dst->unscored, L * 4, "dst->unscored" } };
        { mtr_status st = check_device_cols(ctx, cols, "the column's bytes"); if (st != MTR_OK) return st; }
    }
    a.score = dst->score; a.best = dst->best; a.margin = dst->margin; a.raw = dst->raw; a.pl = dst->pl; a.gt = dst->gt; a.gq = dst->gq; a.scored = dst->scored; a.unscored = dst->unscored;
    if (S > 0) {
        const int64_t P = 2 * S;
        hipLaunchKernelGGL(mtr_k_gq_tasks, dim3((unsigned)std::min<int64_t>((P + GQ_BLOCK - 1) / GQ_BLOCK, GQ_MAX_GRID)), blk, 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        unsigned n[SQ_STATE];
        HIPCHK(copy_sync(ctx, n, c.state, sizeof n, hipMemcpyDeviceToHost));
        if ((int64_t)n[0] + n[1] > P || (int64_t)n[2] + n[3] > P) { ctx->err = "the genotype quality's task lists failed on the device"; return MTR_ERR_HIP; }
        const char *e = getenv("MTR_TEST_GQ_ROWS");
        if (e && atoi(e) == 0) { gq_score_bucket<1, 1>(ctx, a, a.tasks, 1, n[0]); gq_score_bucket<1, 1>(ctx, a, a.tasks + P - 1, -1, n[1]); }
        else { gq_score_bucket<4, 1>(ctx, a, a.tasks, 1, n[0]); gq_score_bucket<2, 1>(ctx, a, a.tasks + P - 1, -1, n[1]); }
        gq_score_bucket<1, 1>(ctx, a, a.tasks + P, 1, n[2]);
        gq_score_bucket<1, 2>(ctx, a, a.tasks + 2 * P - 1, -1, n[3]);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mtr_k_gq_locus, dim3((unsigned)std::min<int64_t>(n_loci, GQ_MAX_GRID)), dim3(64), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}
