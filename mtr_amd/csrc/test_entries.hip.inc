// test_entries.hip.inc — the entry points of include/mtr_hip_test.h (mtr_test_*), included by mtr_abi.hip below everything they reach for (align_host.hip.inc)
extern "C" mtr_status mtr_test_report_lines(mtr_ctx *ctx, int32_t n_rows, const int32_t *fields, const int32_t *read_len, const uint8_t *units,
                                            const int64_t *unit_off, const char *ids, const int64_t *id_off, uint8_t **out_text, int64_t **out_off)
{
    if (!ctx || n_rows < 0 || !unit_off || !id_off || !out_text || !out_off) return MTR_ERR_BAD_ARG;
    if (n_rows > 0 && (!fields || !read_len)) return MTR_ERR_BAD_ARG;
    if (unit_off[0] != 0 || id_off[0] != 0) { ctx->err = "unit_off[0] and id_off[0] must be 0"; return MTR_ERR_BAD_ARG; }
    for (int k = 0; k < n_rows; k++)
        if (unit_off[k + 1] < unit_off[k] || unit_off[k + 1] - unit_off[k] > (1 << 24) || id_off[k + 1] < id_off[k]) { ctx->err = "bad row " + std::to_string(k); return MTR_ERR_BAD_ARG; }
    const size_t nr = (size_t)n_rows, ub = (size_t)unit_off[nr], ib = (size_t)id_off[nr];
    if ((ub > 0 && !units) || (ib > 0 && !ids)) return MTR_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HostArray<int64_t> off = host_array<int64_t>(nr + 1);
    if (!off) return MTR_ERR_OOM;
    off[0] = 0;
    int64_t B = 0;
    if (n_rows > 0) {
        // d_t_i32: fields | read_len;  d_t_units: units | ids;  d_t_i64: unit_off | id_off | bytes | byte_off
        HIPCHK(ctx->d_t_i32.ensure(nr * 15 * 4)); HIPCHK(ctx->d_t_units.ensure(ub + ib + 16)); HIPCHK(ctx->d_t_i64.ensure((4 * nr + 3) * 8));
        int32_t *d_f = ctx->d_t_i32, *d_len = d_f + 14 * nr;
        uint8_t *d_units = ctx->d_t_units, *d_ids = d_units + ub;
        int64_t *d_uoff = ctx->d_t_i64, *d_ioff = d_uoff + nr + 1, *d_bytes = d_ioff + nr + 1, *d_boff = d_bytes + nr;
        HIPCHK(copy_sync(ctx, d_f, fields, nr * 14 * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_len, read_len, nr * 4, hipMemcpyHostToDevice));
        if (ub > 0) HIPCHK(copy_sync(ctx, d_units, units, ub, hipMemcpyHostToDevice));
        if (ib > 0) HIPCHK(copy_sync(ctx, d_ids, ids, ib, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, d_uoff, unit_off, (nr + 1) * 8, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_ioff, id_off, (nr + 1) * 8, hipMemcpyHostToDevice));
        const unsigned blocks = (unsigned)((nr + 63) / 64);
        hipLaunchKernelGGL(mtr_k_text_rows<false>, dim3(blocks), dim3(64), 0, ctx->stream, n_rows, (const int32_t *)d_f, (const int32_t *)d_len, (const uint8_t *)d_units,
                           (const int64_t *)d_uoff, (const uint8_t *)d_ids, (const int64_t *)d_ioff, d_bytes, (const int64_t *)d_boff, (uint8_t *)nullptr);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mtr_k_scan_offsets<int64_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int64_t *)d_bytes, (int64_t)n_rows, d_boff);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_sync(ctx, off.get(), d_boff, (nr + 1) * 8, hipMemcpyDeviceToHost));
        B = off[nr];
        HIPCHK(ctx->d_t_text.ensure((size_t)B + 16));
        hipLaunchKernelGGL(mtr_k_text_rows<true>, dim3(blocks), dim3(64), 0, ctx->stream, n_rows, (const int32_t *)d_f, (const int32_t *)d_len, (const uint8_t *)d_units,
                           (const int64_t *)d_uoff, (const uint8_t *)d_ids, (const int64_t *)d_ioff, d_bytes, (const int64_t *)d_boff, (uint8_t *)ctx->d_t_text);
        HIPCHK(hipGetLastError());
    }
    HostArray<uint8_t> text = host_array<uint8_t>((size_t)std::max<int64_t>(B, 1));
    if (!text) return MTR_ERR_OOM;
    if (B > 0) HIPCHK(copy_sync(ctx, text.get(), ctx->d_t_text, (size_t)B, hipMemcpyDeviceToHost));
    *out_text = text.release(); *out_off = off.release();
    return MTR_OK;
}

extern "C" mtr_status mtr_test_chain(mtr_ctx *ctx, int32_t n_sets, const int64_t *set_off, const int32_t *start, const int32_t *end,
                                     const int32_t *matches, int32_t **out_len, int32_t **out_idx)
{
    if (!ctx || n_sets < 0 || !set_off || !out_len || !out_idx) return MTR_ERR_BAD_ARG;
    if (set_off[0] != 0) { ctx->err = "set_off[0] must be 0"; return MTR_ERR_BAD_ARG; }
    for (int k = 0; k < n_sets; k++)
        if (set_off[k + 1] < set_off[k] || set_off[k + 1] - set_off[k] > (1 << 24)) { ctx->err = "bad set " + std::to_string(k); return MTR_ERR_BAD_ARG; }
    const int64_t total = set_off[n_sets];
    if (total > 0 && (!start || !end || !matches)) return MTR_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    HostArray<int32_t> len = host_array<int32_t>((size_t)std::max(n_sets, 1)), idx = host_array<int32_t>((size_t)std::max<int64_t>(total, 1));
    if (!len || !idx) return MTR_ERR_OOM;
    if (n_sets > 0) {
        std::vector<int64_t> off((size_t)2 * n_sets + 1);              // set offsets | scratch offsets
        int64_t scr = 0;
        for (int k = 0; k <= n_sets; k++) off[(size_t)k] = set_off[k];
        for (int k = 0; k < n_sets; k++) {
            const int64_t c = set_off[k + 1] - set_off[k];
            off[(size_t)n_sets + 1 + k] = c > MTR_CHAIN_LDS_RECS ? scr : -1;
            if (c > MTR_CHAIN_LDS_RECS) scr += MTR_CHAIN_INTS(c);
        }
        const size_t t = (size_t)total;
        HIPCHK(ctx->d_t_i32.ensure((3 * t + 1) * 4)); HIPCHK(ctx->d_t_out.ensure((t + (size_t)n_sets) * 4));
        HIPCHK(ctx->d_ch_scr.ensure((size_t)std::max<int64_t>(scr, 1) * 4)); HIPCHK(ctx->d_t_i64.ensure(off.size() * 8));
        int32_t *d_in = ctx->d_t_i32, *d_out = ctx->d_t_out;
        if (t > 0) {
            HIPCHK(copy_sync(ctx, d_in, start, t * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_in + t, end, t * 4, hipMemcpyHostToDevice));
            HIPCHK(copy_sync(ctx, d_in + 2 * t, matches, t * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(copy_sync(ctx, ctx->d_t_i64, off.data(), off.size() * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(mtr_k_chain_sets, dim3((unsigned)n_sets), dim3(64), 0, ctx->stream, d_in, d_in + t, d_in + 2 * t, ctx->d_t_i64, n_sets,
                           ctx->d_t_i64 + n_sets + 1, ctx->d_ch_scr, d_out, d_out + t);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_sync(ctx, len.get(), d_out + t, (size_t)n_sets * 4, hipMemcpyDeviceToHost));
        if (t > 0) HIPCHK(copy_sync(ctx, idx.get(), d_out, t * 4, hipMemcpyDeviceToHost));
    }
    *out_len = len.release(); *out_idx = idx.release();
    return MTR_OK;
}

extern "C" mtr_status mtr_test_unit_motifs(mtr_ctx *ctx, int32_t n, const char *units, const int64_t *unit_off, const int32_t *read, const int32_t *copies,
                                           const int32_t *repeat_len, int64_t table_slots, uint8_t **strand, int32_t **rotation, int32_t **motif_len, int32_t **group,
                                           int64_t *out_groups, int64_t **motif_off, uint8_t **motifs, int32_t **g_first, int32_t **g_repeats, int32_t **g_reads,
                                           int64_t **g_copies, int64_t **g_bases)
{
    if (!ctx || n < 0 || !unit_off || !strand || !rotation || !motif_len || !group || !out_groups || !motif_off || !motifs || !g_first || !g_repeats || !g_reads ||
        !g_copies || !g_bases) return MTR_ERR_BAD_ARG;
    if (n > 0 && (!read || !copies || !repeat_len)) return MTR_ERR_BAD_ARG;
    if (n > INT32_MAX / 2) { ctx->err = "too many units"; return MTR_ERR_BAD_ARG; }
    if (unit_off[0] != 0) { ctx->err = "unit_off[0] must be 0"; return MTR_ERR_BAD_ARG; }
    if (table_slots != 0 && (table_slots <= n || table_slots > ((int64_t)1 << 31) || (table_slots & (table_slots - 1)) != 0)) {
        ctx->err = "table_slots must be 0 or a power of two above the number of units"; return MTR_ERR_BAD_ARG;
    }
    for (int k = 0; k < n; k++) {
        if (unit_off[k + 1] < unit_off[k] || unit_off[k + 1] - unit_off[k] > MTR_MAX_PERIOD) { ctx->err = "unit " + std::to_string(k) + ": length outside 0..500"; return MTR_ERR_BAD_ARG; }
        if (k > 0 && read[k] < read[k - 1]) { ctx->err = "read decreases at unit " + std::to_string(k); return MTR_ERR_BAD_ARG; }
    }
    const size_t nr = (size_t)n, ub = (size_t)unit_off[nr];
    if (ub > 0 && !units) return MTR_ERR_BAD_ARG;
    for (size_t b = 0; b < ub; b++)
        if (units[b] != 'A' && units[b] != 'C' && units[b] != 'G' && units[b] != 'T') { ctx->err = "byte " + std::to_string(b) + " of the units is none of ACGT"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->mo_ready = false;                                        // the catalogue's buffers are used: a resident batch makes its own again
    MotifWork w{};
    { mtr_status st = motif_work(ctx, n, (int64_t)ub, w); if (st != MTR_OK) return st; }
    if (n > 0) {
        // d_t_units: units;  d_t_i64: unit_off;  d_t_i32: read | copies | repeat_len
        HIPCHK(ctx->d_t_units.ensure(ub + 16)); HIPCHK(ctx->d_t_i64.ensure((nr + 1) * 8)); HIPCHK(ctx->d_t_i32.ensure(3 * nr * 4));
        int32_t *d_in = ctx->d_t_i32;
        if (ub > 0) HIPCHK(copy_sync(ctx, ctx->d_t_units, units, ub, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, ctx->d_t_i64, unit_off, (nr + 1) * 8, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, d_in, read, nr * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_in + nr, copies, nr * 4, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, d_in + 2 * nr, repeat_len, nr * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(mtr_k_unit_motif_rows, dim3((unsigned)((nr + MOTIF_TILE - 1) / MOTIF_TILE)), dim3(64), 0, ctx->stream, n, (const uint8_t *)ctx->d_t_units,
                           (const int64_t *)ctx->d_t_i64, (const int32_t *)d_in, (const int32_t *)(d_in + nr), (const int32_t *)(d_in + 2 * nr), w.rows);
        HIPCHK(hipGetLastError());
    }
    { mtr_status st = motif_group(ctx, n, table_slots, w); if (st != MTR_OK) return st; }
    const size_t g = (size_t)ctx->mo_groups, mb = (size_t)ctx->mo_motif_bytes, n1 = std::max<size_t>(nr, 1), g1 = std::max<size_t>(g, 1);
    const MotifGroups mg = motif_groups(ctx, w);
    HostArray<uint8_t> h_strand = host_array<uint8_t>(n1), h_motifs = host_array<uint8_t>(std::max<size_t>(mb, 1));
    HostArray<int32_t> h_rot = host_array<int32_t>(n1), h_len = host_array<int32_t>(n1), h_group = host_array<int32_t>(n1);
    HostArray<int32_t> h_first = host_array<int32_t>(g1), h_repeats = host_array<int32_t>(g1), h_reads = host_array<int32_t>(g1);
    HostArray<int64_t> h_off = host_array<int64_t>(g + 1), h_copies = host_array<int64_t>(g1), h_bases = host_array<int64_t>(g1);
    if (!h_strand || !h_motifs || !h_rot || !h_len || !h_group || !h_first || !h_repeats || !h_reads || !h_off || !h_copies || !h_bases) return MTR_ERR_OOM;
    const hipMemcpyKind dh = hipMemcpyDeviceToHost;
    HIPCHK(copy_sync(ctx, h_off.get(), mg.motif_off, (g + 1) * 8, dh));
    if (n > 0) {
        HIPCHK(copy_sync(ctx, h_strand.get(), w.rows.strand, nr, dh)); HIPCHK(copy_sync(ctx, h_rot.get(), w.rows.rotation, nr * 4, dh));
        HIPCHK(copy_sync(ctx, h_len.get(), w.rows.motif_len, nr * 4, dh)); HIPCHK(copy_sync(ctx, h_group.get(), mg.group, nr * 4, dh));
        HIPCHK(copy_sync(ctx, h_first.get(), mg.first, g * 4, dh)); HIPCHK(copy_sync(ctx, h_repeats.get(), mg.repeats, g * 4, dh));
        HIPCHK(copy_sync(ctx, h_reads.get(), mg.reads, g * 4, dh)); HIPCHK(copy_sync(ctx, h_copies.get(), mg.copies, g * 8, dh));
        HIPCHK(copy_sync(ctx, h_bases.get(), mg.bases, g * 8, dh));
        if (mb > 0) HIPCHK(copy_sync(ctx, h_motifs.get(), mg.motifs, mb, dh));
    }
    *out_groups = (int64_t)g;
    *strand = h_strand.release(); *rotation = h_rot.release(); *motif_len = h_len.release(); *group = h_group.release();
    *motif_off = h_off.release(); *motifs = h_motifs.release(); *g_first = h_first.release(); *g_repeats = h_repeats.release(); *g_reads = h_reads.release();
    *g_copies = h_copies.release(); *g_bases = h_bases.release();
    return MTR_OK;
}

// the range lists of the resident batch (d_rcount, d_rstart, d_rend, d_rw, d_rdi) as mtr_test_ranges' and mtr_test_ranges_parts' malloc'ed arrays
static mtr_status ranges_to_host(mtr_ctx *ctx, int32_t **out_counts, int32_t **out_start, int32_t **out_end, int32_t **out_w, uint64_t **out_di_bits, int64_t *out_total)
{
    const int n = ctx->n_reads;
    std::vector<int32_t> cnt((size_t)n), st((size_t)ctx->total_rcap), en((size_t)ctx->total_rcap), ww((size_t)ctx->total_rcap);
    std::vector<uint64_t> di((size_t)ctx->total_rcap);
    HIPCHK(copy_sync(ctx, cnt.data(), ctx->d_rcount, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, st.data(), ctx->d_rstart, st.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, en.data(), ctx->d_rend, en.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, ww.data(), ctx->d_rw, ww.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, di.data(), ctx->d_rdi, di.size() * 8, hipMemcpyDeviceToHost));
    int64_t total = 0; for (int i = 0; i < n; i++) total += cnt[(size_t)i];
    const size_t m = (size_t)std::max<int64_t>(total, 1);
    HostArray<int32_t> oc = host_array<int32_t>((size_t)n), os = host_array<int32_t>(m), oe = host_array<int32_t>(m), ow = host_array<int32_t>(m);
    HostArray<uint64_t> od = host_array<uint64_t>(m);
    if (!oc || !os || !oe || !ow || !od) return MTR_ERR_OOM;
    int64_t p = 0;
    for (int i = 0; i < n; i++) {
        oc[i] = cnt[(size_t)i];
        for (int t = 0; t < cnt[(size_t)i]; t++, p++) {
            size_t q = (size_t)ctx->roff[(size_t)i] + (size_t)t;
            os[p] = st[q]; oe[p] = en[q]; ow[p] = ww[q]; od[p] = di[q];
        }
    }
    *out_counts = oc.release(); *out_start = os.release(); *out_end = oe.release(); *out_w = ow.release(); *out_di_bits = od.release(); if (out_total) *out_total = total;
    return MTR_OK;
}

extern "C" mtr_status mtr_test_ranges(mtr_ctx *ctx, int32_t **out_counts, int32_t **out_start, int32_t **out_end,
                                      int32_t **out_w, uint64_t **out_di_bits, int64_t *out_total)
{
    if (!ctx || !out_counts || !out_start || !out_end || !out_w || !out_di_bits) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    HIPCHK(hipMemsetAsync(ctx->d_status, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned long long) * CNT_N, ctx->stream));
    mtr_status s = launch_k1(ctx); if (s != MTR_OK) return s;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1])); ctx->kt[0].ms = ms; ctx->kt[0].launches = 1;
    s = check_status(ctx); if (s != MTR_OK) return s;
    return ranges_to_host(ctx, out_counts, out_start, out_end, out_w, out_di_bits, out_total);
}

// The range finder as the staged chain runs it on a batch of few reads: launch_k1_parts alone, under launch_staged's own conditions for it
extern "C" mtr_status mtr_test_ranges_parts(mtr_ctx *ctx, int32_t **out_counts, int32_t **out_start, int32_t **out_end,
                                            int32_t **out_w, uint64_t **out_di_bits, int64_t *out_total)
{
    if (!ctx || !out_counts || !out_start || !out_end || !out_w || !out_di_bits) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    const int n = ctx->n_reads;
    const int parts_max = 256;                               // launch_staged's parts_max
    if (n > parts_max) {
        ctx->err = "a batch of " + std::to_string(n) + " reads: the staged chain runs the three-kernel range finder on at most " + std::to_string(parts_max);
        return MTR_ERR_BAD_ARG;
    }
    const K1Layout y1 = k1_layout(ctx->Lmax);
    size_t tot = 0;
    if (pick_waves(ctx, n, n, y1.total, &tot) != n) {
        ctx->err = "per-read scratch of " + std::to_string(n) + " x " + std::to_string(y1.total) + " bytes does not fit: the staged chain would not run the three-kernel range finder on this batch";
        return MTR_ERR_BAD_ARG;
    }
    HIPCHK(hipMemsetAsync(ctx->d_status, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned long long) * CNT_N, ctx->stream));
    // launch_k1_parts records no events: the entry's own pair around everything it enqueues (the item lists' copies included)
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    mtr_status s = launch_k1_parts(ctx); if (s != MTR_OK) return s;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int passes = 0; for (int i = 0; i < n; i++) passes += k1_num_passes(ctx->lens[(size_t)i]);
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1])); ctx->kt[0].ms = ms; ctx->kt[0].launches = passes > 0 ? 3 : 2;
    s = check_status(ctx); if (s != MTR_OK) return s;
    return ranges_to_host(ctx, out_counts, out_start, out_end, out_w, out_di_bits, out_total);
}

extern "C" mtr_status mtr_test_file_tail(mtr_ctx *ctx, uint16_t **out_tail, int64_t **out_tail_off, uint8_t **out_after)
{
    if (!ctx || !out_tail || !out_tail_off || !out_after) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->n_reads;
    const int64_t entries = ctx->file_order ? ctx->tail_entries : 0;
    HostArray<uint16_t> tl = host_array<uint16_t>((size_t)std::max<int64_t>(entries, 1));
    HostArray<int64_t> to = host_array<int64_t>(n + 1);
    HostArray<uint8_t> af = host_array<uint8_t>(n * 2);
    if (!tl || !to || !af) return MTR_ERR_OOM;
    tl[0] = 0; memset(to.get(), 0, (n + 1) * 8); memset(af.get(), 0, n * 2);
    if (ctx->file_order) {
        HIPCHK(copy_sync(ctx, to.get(), ctx->d_tail_off, (n + 1) * 8, hipMemcpyDeviceToHost));
        if (entries > 0) HIPCHK(copy_sync(ctx, tl.get(), ctx->d_tail, (size_t)entries * 2, hipMemcpyDeviceToHost));
        if (ctx->after.size() >= n * 2) memcpy(af.get(), ctx->after.data(), n * 2);
    }
    // id 0 of mtr_get_kernel_times: mtr_k_file_tail of this batch's upload (launches = 0: a host upload, or no tail entry)
    ctx->kt[0].ms = ctx->file_order ? ctx->fo_tail_ms : 0; ctx->kt[0].launches = ctx->file_order ? ctx->fo_tail_launches : 0;
    *out_tail = tl.release(); *out_tail_off = to.release(); *out_after = af.release();
    return MTR_OK;
}

// mtr_test_wrap_dp's and mtr_test_wrap_dp_pass's tasks: the caller's arrays into the table of d_t_i32 (group_off behind it), the units into d_t_units, `a` from its columns
struct DpTestTasks { const int32_t *read_idx, *query_start, *query_end, *gain, *mismatch, *indel, *unit_off; const uint8_t *units; };
static mtr_status dp_test_upload(mtr_ctx *ctx, const DpTestTasks &h, size_t nt, size_t out_ints, const int32_t *group_off, size_t ng, DpTestArgs &a, const int32_t **d_group_off)
{
    const size_t ub = (size_t)h.unit_off[nt];
    HIPCHK(ctx->d_t_i32.ensure((group_off ? dp_task_ints(nt, ng) : dp_task_ints(nt)) * 4)); HIPCHK(ctx->d_t_units.ensure(ub + 16)); HIPCHK(ctx->d_t_out.ensure(nt * out_ints * 4));
    const DpTaskTable<int32_t> t = dp_task_table<int32_t>(ctx->d_t_i32, nt);
    HIPCHK(copy_sync(ctx, t.read, h.read_idx, nt * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, t.start, h.query_start, nt * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, t.end, h.query_end, nt * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, t.gain, h.gain, nt * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, t.mism, h.mismatch, nt * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, t.indel, h.indel, nt * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, t.unit_off, h.unit_off, (nt + 1) * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, ctx->d_t_units, h.units, ub, hipMemcpyHostToDevice));
    if (group_off) HIPCHK(copy_sync(ctx, t.group_off, group_off, (ng + 1) * 4, hipMemcpyHostToDevice));
    a.b = view(ctx); a.n_tasks = (int32_t)nt; a.read_idx = t.read; a.qs = t.start; a.qe = t.end; a.units = ctx->d_t_units; a.unit_off = t.unit_off;
    a.gain = t.gain; a.mism = t.mism; a.indel = t.indel; a.out8 = ctx->d_t_out;
    if (d_group_off) *d_group_off = t.group_off;
    return MTR_OK;
}

extern "C" mtr_status mtr_test_wrap_dp(mtr_ctx *ctx, int32_t n_tasks, const int32_t *read_idx, const int32_t *query_start,
                                       const int32_t *query_end, const uint8_t *units, const int32_t *unit_off,
                                       const int32_t *gain, const int32_t *mismatch, const int32_t *indel, int32_t *out8)
{
    if (!ctx || n_tasks <= 0 || !read_idx || !query_start || !query_end || !units || !unit_off || !gain || !mismatch || !indel || !out8) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    size_t cells = 1;
    for (int t = 0; t < n_tasks; t++) {
        int rd = read_idx[t];
        int U = unit_off[t + 1] - unit_off[t];
        if (rd < 0 || rd >= ctx->n_reads || query_start[t] < 0 || query_end[t] < query_start[t] || query_end[t] >= ctx->lens[(size_t)rd] || U <= 0 || U >= MTRC_MAX_PERIOD) { ctx->err = "bad DP task " + std::to_string(t); return MTR_ERR_BAD_ARG; }
        cells = std::max(cells, (size_t)(query_end[t] - query_start[t] + 1) * (size_t)(U + 1));   // rows may be padded to an even length
    }
    DpScratch sc; { mtr_status s = dp_scratch(ctx, dp_matrix_bytes(cells), n_tasks, sc); if (s != MTR_OK) return s; }
    DBG("test_wrap_dp: %d tasks, cells %zu, waves %d, scratch %zu", n_tasks, cells, sc.waves, sc.total);
    const size_t nt = (size_t)n_tasks; DpTestArgs a{};
    { mtr_status s = dp_test_upload(ctx, { read_idx, query_start, query_end, gain, mismatch, indel, unit_off, units }, nt, 8, nullptr, 0, a, nullptr); if (s != MTR_OK) return s; }
    { mtr_status s = dp_launch_reset(ctx, a, sc.per_wave, cells, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream)); DBG("test_wrap_dp: launching");
    hipLaunchKernelGGL(mtr_k_dp_test, dim3((unsigned)sc.waves), dim3(64), 0, ctx->stream, a);
    HIPCHK(hipGetLastError()); HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    { mtr_status s = dp_launch_wait(ctx, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }
    DBG("test_wrap_dp: kernel done");
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3])); ctx->kt[1].ms = ms; ctx->kt[1].launches = 1;
    HIPCHK(copy_sync(ctx, out8, a.out8, nt * 8 * 4, hipMemcpyDeviceToHost));
    return check_status(ctx);
}

// polish_repeat alone, a task per wavefront turn (dp_test.hip.inc: mtr_k_polish_test), on the narrow scratch layout of the chain's polish kernel
extern "C" mtr_status mtr_test_polish(mtr_ctx *ctx, int32_t n_tasks, const int32_t *read_idx, const int32_t *rep_start, const int32_t *rep_end,
                                      const int32_t *k, const uint8_t *units, const int32_t *scores, const int32_t *unit_off,
                                      uint8_t *out_units, int32_t *out_len)
{
    if (!ctx || n_tasks <= 0 || !read_idx || !rep_start || !rep_end || !k || !units || !scores || !unit_off || !out_units || !out_len) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    if (unit_off[0] != 0) { ctx->err = "unit_off[0] is not 0"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    for (int t = 0; t < n_tasks; t++) {
        const int rd = read_idx[t], U = unit_off[t + 1] - unit_off[t];
        if (rd < 0 || rd >= ctx->n_reads || rep_start[t] < 0 || rep_end[t] < rep_start[t] || rep_end[t] >= ctx->lens[(size_t)rd] || U <= 0 || U >= MTRC_MAX_PERIOD ||
            k[t] < 2 || k[t] > MTRC_MAX_KMER) { ctx->err = "bad polish task " + std::to_string(t); return MTR_ERR_BAD_ARG; }
    }
    const size_t nt = (size_t)n_tasks, ub = (size_t)unit_off[n_tasks];
    const size_t per_wave = k2_layout(ctx->Lmax, 256).total;
    DpScratch sc; { mtr_status s = dp_scratch(ctx, per_wave, n_tasks, sc); if (s != MTR_OK) return s; }
    // d_t_i32: read | rep_start | rep_end | k | unit_off | scores;  d_t_out: lengths | units
    HIPCHK(ctx->d_t_i32.ensure((nt * 5 + 1 + ub) * 4)); HIPCHK(ctx->d_t_units.ensure(ub + 16)); HIPCHK(ctx->d_t_out.ensure(nt * 4 + nt * MTRC_MAX_PERIOD + 16));
    int32_t *d_i32 = ctx->d_t_i32; uint8_t *d_units = ctx->d_t_units; int32_t *d_len = ctx->d_t_out; uint8_t *d_out = (uint8_t *)(d_len + nt);
    int32_t *d_rd = d_i32, *d_rs = d_i32 + nt, *d_re = d_i32 + 2 * nt, *d_k = d_i32 + 3 * nt, *d_uo = d_i32 + 4 * nt, *d_sc = d_i32 + 5 * nt + 1;
    HIPCHK(copy_sync(ctx, d_rd, read_idx, nt * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_rs, rep_start, nt * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, d_re, rep_end, nt * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_k, k, nt * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, d_uo, unit_off, (nt + 1) * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_sc, scores, ub * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, d_units, units, ub, hipMemcpyHostToDevice));
    PolishTestArgs p{}; k2_args(ctx, p.a, per_wave); p.a.trace_cap = 0;
    p.n_tasks = n_tasks; p.read_idx = d_rd; p.rep_start = d_rs; p.rep_end = d_re; p.k = d_k; p.units = d_units; p.scores = d_sc; p.unit_off = d_uo;
    p.out_units = d_out; p.out_len = d_len;
    { mtr_status s = dp_launch_reset(ctx, p.a, per_wave, 256, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }        // (256: the narrow layout's cell region, k2_layout)
    hipLaunchKernelGGL(mtr_k_polish_test, dim3((unsigned)sc.waves), dim3(64), 0, ctx->stream, p);
    { mtr_status s = dp_launch_wait(ctx, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }
    HIPCHK(copy_sync(ctx, out_len, d_len, nt * 4, hipMemcpyDeviceToHost)); HIPCHK(copy_sync(ctx, out_units, d_out, nt * MTRC_MAX_PERIOD, hipMemcpyDeviceToHost));
    return check_status(ctx);
}

// One chosen forward pass on chosen groups (dp_test.hip.inc).  The host holds every task to the bounds under which the batch path hands a DP to that
// pass - the same macros, evaluated here - and refuses the rest before anything is launched.
extern "C" mtr_status mtr_test_wrap_dp_pass(mtr_ctx *ctx, int32_t pass, int32_t n_groups, const int32_t *group_off, const int32_t *read_idx,
                                            const int32_t *query_start, const int32_t *query_end, const uint8_t *units, const int32_t *unit_off,
                                            const int32_t *gain, const int32_t *mismatch, const int32_t *indel, int32_t *out16)
{
    if (!ctx || pass < MTR_TEST_PASS_WAVE2P || pass > MTR_TEST_PASS_OCT2P || n_groups <= 0 || !group_off || !read_idx || !query_start || !query_end || !units || !unit_off ||
        !gain || !mismatch || !indel || !out16) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    if (group_off[0] != 0) { ctx->err = "group_off[0] is not 0"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    const long long lim16 = ctx->sw.dp16_max_rows;
    const bool one_param = pass == MTR_TEST_PASS_FOUR1P || pass == MTR_TEST_PASS_OCT1P;
    const int max_members = pass == MTR_TEST_PASS_WAVE2P ? 1 : pass == MTR_TEST_PASS_OCT1P ? RQ_SLOTS : pass == MTR_TEST_PASS_OCT2P ? 8 : 4;
    auto refuse = [&](int g, int t, const char *why) {
        ctx->err = "bad DP pass task " + std::to_string(t) + " (group " + std::to_string(g) + "): " + why; return MTR_ERR_BAD_ARG;
    };
    auto size_ok = [&](long long U, long long rows) { return (U + 1) * rows + U < ctx->wrap_dp_size; };       // dp_size_ok (device_util.hip.inc)
    size_t cells = 1;                                        // the largest cell block of a group
    int quad_cols = 0;
    for (int g = 0; g < n_groups; g++) {
        const int t0 = group_off[g], n = group_off[g + 1] - t0;
        if (t0 < 0 || n < 1 || n > max_members) return refuse(g, t0, "empty group, or more members than the pass takes");
        long long maxrows = 0, maxU = 0, sumU = 0;
        for (int t = t0; t < t0 + n; t++) {
            const int rd = read_idx[t];
            const long long U = (long long)unit_off[t + 1] - unit_off[t];
            if (rd < 0 || rd >= ctx->n_reads || query_start[t] < 0 || query_end[t] < query_start[t] || query_end[t] >= ctx->lens[(size_t)rd]) return refuse(g, t, "window outside its read");
            if (U <= 0 || U >= MTRC_MAX_PERIOD) return refuse(g, t, "unit length");
            const long long rows = (long long)query_end[t] - query_start[t] + 1;
            if (!size_ok(U, rows)) return refuse(g, t, "beyond WrapDPsize");
            switch (pass) {
            case MTR_TEST_PASS_WAVE2P: break;                // dp_two_params_unit takes every alignment
            case MTR_TEST_PASS_Q4:                           // dp_batch_fits + the units the pool batches
                if (U > 16) return refuse(g, t, "unit above 16 bases");
                if (rows > DP2P_MAX_ROWS || rows > lim16 || !size_ok(16, rows)) return refuse(g, t, "rows beyond dp_batch_fits");
                if (rd != read_idx[t0] || query_start[t] != query_start[t0] || query_end[t] != query_end[t0]) return refuse(g, t, "the units of a Q4 group share read and window");
                break;
            case MTR_TEST_PASS_QUAD2P:                       // mtr_k_gather's isq
                if (U > ST_QUMAX) return refuse(g, t, "unit above ST_QUMAX");
                if (rows > DP2P_MAX_ROWS || rows > lim16 || !DPQ_FITS(rows, U, 1, 3)) return refuse(g, t, "rows beyond DPQ_FITS");
                if (quad_cols == 0) quad_cols = DPQ_COLS(U);
                if (DPQ_COLS(U) != quad_cols) return refuse(g, t, "the tasks of a QUAD2P call are of one DPQ_COLS class");
                break;
            case MTR_TEST_PASS_OCT2P:                        // mtr_k_gather's isq, and the units that go eight per wavefront
                if (U > ST_OUMAX) return refuse(g, t, "unit above ST_OUMAX");
                if (rows > DP2P_MAX_ROWS || rows > lim16 || !DPQ_FITS(rows, U, 1, 3)) return refuse(g, t, "rows beyond DPQ_FITS");
                break;
            default: {                                       // mtr_k_revise_quads' fits
                const int G = gain[t], MM = mismatch[t], D = indel[t];
                if (!((G == 1 && MM == 1 && D == 3) || (G == 1 && MM == 3 && D == 1) || (G == 5 && MM == 1 && D == 1))) return refuse(g, t, "not one of the three parameter sets");
                if (U > ST_QUMAX) return refuse(g, t, "unit above ST_QUMAX");
                if (rows > lim16 || !DPQ_FITS(rows, U, G, D)) return refuse(g, t, "rows beyond DPQ_FITS");
                break; }
            }
            maxrows = std::max(maxrows, rows); maxU = std::max(maxU, U); sumU += U;
        }
        size_t block;
        switch (pass) {
        case MTR_TEST_PASS_WAVE2P: block = 2 * (size_t)maxrows * (size_t)(maxU + 1) + 64; break;      // dp_forward2 writes two matrices; a wide row is at most 256 bytes
        case MTR_TEST_PASS_Q4: block = (size_t)maxrows * (size_t)sumU; break;
        case MTR_TEST_PASS_QUAD2P: block = DPQ_BLOCK_BYTES(DPQ_COLS(maxU), maxrows); break;
        case MTR_TEST_PASS_OCT2P: block = DPO_BLOCK_BYTES((maxU + 7) / 8, maxrows); break;
        default: block = (RQ_SLOTS / 4) * DPQP_BLOCK_BYTES(DPQ_COLS(maxU), maxrows); break;
        }
        cells = std::max(cells, block);
    }
    if (dp_matrix_bytes(cells) > scratch_cap(ctx)) { ctx->err = "bad DP pass task: a group's cell block of " + std::to_string(cells) + " bytes exceeds the scratch cap"; return MTR_ERR_BAD_ARG; }
    DpScratch sc; { mtr_status s = dp_scratch(ctx, dp_matrix_bytes(cells), n_groups, sc); if (s != MTR_OK) return s; }
    const size_t nt = (size_t)group_off[n_groups], ng = (size_t)n_groups; DpPassArgs a{};
    { mtr_status s = dp_test_upload(ctx, { read_idx, query_start, query_end, gain, mismatch, indel, unit_off, units }, nt, 16, group_off, ng, a.t, &a.group_off); if (s != MTR_OK) return s; }
    a.pass = pass; a.n_groups = n_groups; a.packed_words = ctx->packed_words;
    { mtr_status s = dp_launch_reset(ctx, a.t, sc.per_wave, cells, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }
    HIPCHK(hipMemsetAsync(a.t.out8, 0, nt * 16 * 4, ctx->stream));
    const dim3 grid((unsigned)sc.waves), block(64);
    if (pass == MTR_TEST_PASS_WAVE2P || pass == MTR_TEST_PASS_Q4) hipLaunchKernelGGL(mtr_k_dp_test_waves, grid, block, 0, ctx->stream, a);
    else if (one_param) hipLaunchKernelGGL(mtr_k_dp_test_rev, grid, block, 0, ctx->stream, a);
    else if (pass == MTR_TEST_PASS_OCT2P) hipLaunchKernelGGL(mtr_k_dp_test_octs, grid, block, 0, ctx->stream, a);
    else {
        typedef void (*quad_kernel)(DpPassArgs);
        static const quad_kernel by_cols[8] = { mtr_k_dp_test_quads<1>, mtr_k_dp_test_quads<2>, mtr_k_dp_test_quads<3>, mtr_k_dp_test_quads<4>,
                                                mtr_k_dp_test_quads<5>, mtr_k_dp_test_quads<6>, mtr_k_dp_test_quads<7>, mtr_k_dp_test_quads<8> };
        hipLaunchKernelGGL(by_cols[quad_cols - 1], grid, block, 0, ctx->stream, a);
    }
    { mtr_status s = dp_launch_wait(ctx, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }
    HIPCHK(copy_sync(ctx, out16, a.t.out8, nt * 16 * 4, hipMemcpyDeviceToHost));
    return check_status(ctx);
}

// revise_representative_unit on chosen records and units (include/mtr_hip_test.h).  WAVE: revise() on one wavefront per group (dp_test.hip.inc:
// mtr_k_revise_test); SLOTS: mtr_k_revise_quads ITSELF over a work list made here in the shape mtr_k_select / mtr_k_polish / mtr_k_rscatter leave it - per task a
// block header (the kernel reads its rd), a revision record with the polished unit and the node frequencies behind it, its arena offset in rev_items, and
// `sorted` in the caller's order.  The host holds every task to the bounds under which the batch path hands a record to its revision (revise_task.h) and refuses
// the rest before anything is launched.  Scratch per wavefront and the cell budget are launch_staged's for the resident batch.
#include "revise_task.h"
extern "C" mtr_status mtr_test_revise(mtr_ctx *ctx, int32_t mode, int32_t n_groups, const int32_t *group_off, const int32_t *read_idx, const int32_t *rr,
                                      const uint8_t *units, const int32_t *scores, const int32_t *unit_off, int32_t waves, int32_t *out_rr, uint8_t *out_units,
                                      int64_t *out_cells)
{
    if (!ctx || (mode != MTR_TEST_REVISE_WAVE && mode != MTR_TEST_REVISE_SLOTS) || waves < 0 || !group_off || !read_idx || !rr || !units || !scores || !unit_off ||
        !out_rr || !out_units || !out_cells) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "bad revision task: no batch uploaded"; return MTR_ERR_BAD_ARG; }
    if (n_groups <= 0) { ctx->err = "bad revision task: no group"; return MTR_ERR_BAD_ARG; }
    if (group_off[0] != 0 || unit_off[0] != 0) { ctx->err = "bad revision task: group_off[0] or unit_off[0] is not 0"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    for (int g = 0; g < n_groups; g++) {
        if (group_off[g + 1] <= group_off[g]) { ctx->err = "bad revision task " + std::to_string(group_off[g]) + " (group " + std::to_string(g) + "): empty group"; return MTR_ERR_BAD_ARG; }
        if (group_off[g + 1] > RVT_MAX_TASKS) { ctx->err = "bad revision task " + std::to_string(RVT_MAX_TASKS) + " (group " + std::to_string(g) + "): more tasks than the lists hold"; return MTR_ERR_BAD_ARG; }
        for (int t = group_off[g]; t < group_off[g + 1]; t++) {
            const int64_t U = (int64_t)unit_off[t + 1] - unit_off[t];
            std::string why = rvt_refusal(read_idx[t], ctx->n_reads, ctx->lens.data(), rr + (size_t)t * 13, U, ctx->wrap_dp_size);
            if (why.empty()) for (int64_t q = 0; q < U; q++) if (units[unit_off[t] + q] > 3) { why = "a unit code above 3"; break; }
            // (the round memo is a range's, and a range lies in one read: its key does not hold the read)
            if (why.empty() && mode == MTR_TEST_REVISE_WAVE && read_idx[t] != read_idx[group_off[g]]) why = "the tasks of a WAVE group share their read";
            if (!why.empty()) { ctx->err = "bad revision task " + std::to_string(t) + " (group " + std::to_string(g) + "): " + why; return MTR_ERR_BAD_ARG; }
        }
    }
    const size_t nt = (size_t)group_off[n_groups], ng = (size_t)n_groups, ub = (size_t)unit_off[nt];
    // launch_staged's scratch per wavefront: the unit layout alone where the three-kernel range finder takes per-read scratch, else the larger of the two
    const int n = ctx->n_reads;
    const K1Layout y1 = k1_layout(ctx->Lmax); const K2Layout y2 = k2_layout(ctx->Lmax);
    bool parts = n <= 256;
    if (parts) { size_t tot = 0; parts = pick_waves(ctx, n, n, y1.total, &tot) == n; }
    const size_t per_wave = parts ? y2.total : std::max(y1.total, y2.total);
    *out_cells = (int64_t)y2.cells;
    const bool slots = mode == MTR_TEST_REVISE_SLOTS;
    const int want = waves > 0 ? waves : slots ? 1 : (int)std::min<size_t>(ng, 1u << 20);
    size_t total = 0;
    const int nw = pick_waves(ctx, slots ? want : std::min<int>(want, (int)ng), slots ? 32 : 8, per_wave, &total);
    { mtr_status s = ensure_scratch(ctx, total); if (s != MTR_OK) return s; }
    K2Args a{}; k2_args(ctx, a, per_wave); a.trace_cap = 0;
    { mtr_status s = dp_launch_reset(ctx, a, per_wave, 0, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }      // (cells_cap 0: the whole cell region, as the chain's DP kernels have it)
    if (!slots) {
        // d_t_i32: group_off | read_idx | rr | unit_off | scores;  d_t_out: records | units
        HIPCHK(ctx->d_t_i32.ensure((ng + 1 + nt + 13 * nt + nt + 1 + ub) * 4)); HIPCHK(ctx->d_t_units.ensure(ub + 16)); HIPCHK(ctx->d_t_out.ensure(nt * 13 * 4 + nt * MTRC_MAX_PERIOD + 16));
        int32_t *d_go = ctx->d_t_i32, *d_rd = d_go + ng + 1, *d_rr = d_rd + nt, *d_uo = d_rr + 13 * nt, *d_sc = d_uo + nt + 1;
        int32_t *d_orr = ctx->d_t_out; uint8_t *d_ou = (uint8_t *)(d_orr + 13 * nt);
        HIPCHK(copy_sync(ctx, d_go, group_off, (ng + 1) * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_rd, read_idx, nt * 4, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, d_rr, rr, nt * 13 * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_uo, unit_off, (nt + 1) * 4, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, d_sc, scores, ub * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, ctx->d_t_units, units, ub, hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(d_orr, 0, nt * 13 * 4 + nt * MTRC_MAX_PERIOD, ctx->stream));
        ReviseTestArgs p{}; p.a = a; p.n_groups = n_groups; p.group_off = d_go; p.read_idx = d_rd; p.rr = d_rr; p.units = ctx->d_t_units; p.scores = d_sc; p.unit_off = d_uo;
        p.out_rr = d_orr; p.out_units = d_ou;
        hipLaunchKernelGGL(mtr_k_revise_test, dim3((unsigned)nw), dim3(64), 0, ctx->stream, p);
        { mtr_status s = dp_launch_wait(ctx, DP_COUNTERS_OWN); if (s != MTR_OK) return s; }
        HIPCHK(copy_sync(ctx, out_rr, d_orr, nt * 13 * 4, hipMemcpyDeviceToHost)); HIPCHK(copy_sync(ctx, out_units, d_ou, nt * MTRC_MAX_PERIOD, hipMemcpyDeviceToHost));
        return check_status(ctx);
    }
    // the work list of mtr_k_revise_quads.  d_t_units: the arena (per task: StItemHdr, StRev, unit, node frequencies);  d_t_i64: rev_items;
    // d_t_i32: sorted | quad_cls;  d_t_out: the work queues
    const size_t block = sizeof(StItemHdr) + (size_t)ST_REV_BYTES, qwords = (size_t)ST_N_QUEUES * WQ_WORDS;
    std::vector<uint8_t> arena(nt * block, 0);
    std::vector<long long> items(nt);
    std::vector<int32_t> lists(nt + 16, 0);
    for (size_t t = 0; t < nt; t++) {
        const size_t base = t * block, ro = base + sizeof(StItemHdr);
        const int U = unit_off[t + 1] - unit_off[t];
        StItemHdr h{}; h.rd = read_idx[t];
        StRev rv{}; rv.block = (long long)base; rv.k = rr[t * 13 + 9]; rv.slot = 0; rv.leader = -1; rv.ri = (int32_t)t;
        for (int f = 0; f < 13; f++) rv.rr[f] = rr[t * 13 + (size_t)f];
        memcpy(arena.data() + base, &h, sizeof h); memcpy(arena.data() + ro, &rv, sizeof rv);
        memcpy(arena.data() + ro + sizeof(StRev), units + unit_off[t], (size_t)U);
        int32_t *sc = (int32_t *)(arena.data() + ro + sizeof(StRev) + K2_SLOT_UNIT);
        for (int q = 0; q < K2_SLOT_SCORE; q++) sc[q] = q < U ? scores[unit_off[t] + q] : -1;
        items[t] = (long long)ro; lists[t] = (int32_t)t;
    }
    lists[nt + ST_QCLASSES] = (int32_t)nt; lists[nt + ST_QCLASSES + 1] = 1;
    HIPCHK(ctx->d_t_units.ensure(arena.size() + 16)); HIPCHK(ctx->d_t_i64.ensure(nt * 8)); HIPCHK(ctx->d_t_i32.ensure(lists.size() * 4)); HIPCHK(ctx->d_t_out.ensure(qwords * 4));
    HIPCHK(copy_sync(ctx, ctx->d_t_units, arena.data(), arena.size(), hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, ctx->d_t_i64, items.data(), nt * 8, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, ctx->d_t_i32, lists.data(), lists.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(ctx->d_t_out, 0, qwords * 4, ctx->stream));
    StagedArgs s{};
    s.n_reads = n; s.arena = ctx->d_t_units; s.arena_cap = (long long)arena.size(); s.rev_items = (long long *)ctx->d_t_i64.p; s.rev_cap = (int32_t)nt;
    s.sorted = ctx->d_t_i32; s.sorted_cap = (int32_t)nt; s.quad_cls = s.sorted + nt; s.work = (unsigned *)ctx->d_t_out.p; s.nsub = 1; s.quad_min = 1;
    hipLaunchKernelGGL(mtr_k_revise_quads, dim3((unsigned)nw), dim3(64), 0, ctx->stream, a, s);
    { mtr_status st = dp_launch_wait(ctx, DP_COUNTERS_OWN); if (st != MTR_OK) return st; }
    HIPCHK(copy_sync(ctx, arena.data(), ctx->d_t_units, arena.size(), hipMemcpyDeviceToHost));
    memset(out_units, 0, nt * MTRC_MAX_PERIOD);
    for (size_t t = 0; t < nt; t++) {
        const size_t ro = t * block + sizeof(StItemHdr);
        StRev rv; memcpy(&rv, arena.data() + ro, sizeof rv);
        for (int f = 0; f < 13; f++) out_rr[t * 13 + (size_t)f] = rv.rr[f];
        const int U = std::max(0, std::min(rv.rr[3], MTRC_MAX_PERIOD));
        memcpy(out_units + t * MTRC_MAX_PERIOD, arena.data() + ro + sizeof(StRev), (size_t)U);
    }
    return check_status(ctx);
}

// ---- the rounds of the last window-edits call (mtr_window_edits_device, allele_host.hip.inc) ----
extern "C" mtr_status mtr_test_window_edits_rounds(mtr_ctx *ctx, int32_t *rounds)
{
    if (!ctx || !rounds) return MTR_ERR_BAD_ARG;
    if (!ctx->we_ready) { ctx->err = "no edits kept: mtr_window_edits_device comes first"; return MTR_ERR_BAD_ARG; }
    *rounds = ctx->we_rounds;
    return MTR_OK;
}
