// align_host.hip.inc — the hosts that hand wrap-around DP work to the kernels: what they share with the motif hosts and the test entry points (layouts and
// sizes: dp_task_plan.h; DESIGN.md 7i-14), then the -a alignments of the report's repeats and of a caller's records.  Included below the report's chains.
struct DpScratch { size_t per_wave; int waves; size_t total; };     // of a launch of wavefronts of per_wave bytes over n_items items, 8 per CU: picked, then grown
static mtr_status dp_scratch(mtr_ctx *ctx, size_t per_wave, int n_items, DpScratch &z) { z = { per_wave, 0, 0 }; z.waves = pick_waves(ctx, n_items, 8, per_wave, &z.total); return ensure_scratch(ctx, z.total); }
// The launch reset: the common tail of an argument struct (AlignArgs, DpTestArgs, K2Args agree on the names), status word and work counter zeroed.  The counters
// differ on purpose: OWN - the three DP test entry points clear them here and read them back (dp_launch_wait); KEPT - mtr_alignments and report_alignments do neither.
enum DpCounters { DP_COUNTERS_KEPT, DP_COUNTERS_OWN };
template <typename Args> static mtr_status dp_launch_reset(mtr_ctx *ctx, Args &a, size_t per_wave, size_t cells_cap, DpCounters counters)
{
    a.scratch = ctx->d_scratch; a.scratch_per_wave = per_wave; a.cells_cap = cells_cap;
    a.status = ctx->d_status; a.work_counter = ctx->d_work; a.counters = ctx->d_counters; a.dp16_max_rows = ctx->sw.dp16_max_rows;
    HIPCHK(hipMemsetAsync(ctx->d_status, 0, 4, ctx->stream)); HIPCHK(hipMemsetAsync(ctx->d_work, 0, sizeof(unsigned), ctx->stream));
    if (counters == DP_COUNTERS_OWN) HIPCHK(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned long long) * CNT_N, ctx->stream));
    return MTR_OK;
}
static mtr_status dp_launch_wait(mtr_ctx *ctx, DpCounters counters)          // the launch enqueued: its error, its end, its counters
{
    HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(ctx->stream));
    if (counters == DP_COUNTERS_OWN) HIPCHK(copy_sync(ctx, ctx->counters, ctx->d_counters, sizeof(unsigned long long) * CNT_N, hipMemcpyDeviceToHost));
    return MTR_OK;
}
// the context's part of the five-launch plan (dp_task_plan.h): its pick is pick_waves of this context
struct DpPick { mtr_ctx *ctx; int operator()(int64_t items, int per_cu, size_t per_wave, size_t *total) const { return pick_waves(ctx, (int)std::min<int64_t>(items, INT32_MAX), per_cu, per_wave, total); } };
// its launches, the scratch grown to p.scratch before: launch(k, grid, block) sets the host's own fields, says its MTR_DEBUG line and enqueues its kernel
template <typename Args, typename Launch> static mtr_status dp_plan_launches(mtr_ctx *ctx, const DpLaunchPlan &p, Args &a, unsigned long long *counters, Launch launch)
{
    for (int k = 0; k < DP_LAUNCHES; k++) {
        if (p.waves[k] == 0) continue;
        a.counter = counters + k; a.scratch_per_wave = p.per_wave[k]; a.cells_cap = p.cells_cap[k];
        launch(k, dim3((unsigned)p.waves[k]), dim3(64)); HIPCHK(hipGetLastError());
    }
    return MTR_OK;
}

// ---- the -a alignments of the report's repeats (report_align.hip.inc) -------------------------------------------------------
// d_ra_sizes: [0, n) path bytes per read | [n, 2n) unit bytes per read | [2n, 3n] offsets of the reads' units | [3n+1, 4n+1] offsets of
// their paths | [4n+2] cells of the largest DP.  Only those closing scalars and the number of columns come to the host.
struct AlignSizes { int64_t *read_cap, *read_units, *unit_base, *cap_base, *max_cells; };
static AlignSizes align_sizes(int64_t *base, int n) { return { base, base + n, base + 2 * n, base + 3 * n + 1, base + 4 * n + 2 }; }

// mtr_k_align over the n tasks of the table at d_i32, `a` holding the units and where the paths go; cells: the largest DP's
static mtr_status launch_align(mtr_ctx *ctx, AlignArgs &a, int32_t n, int32_t *d_i32, size_t cells, const DpScratch &sc)
{
    const DpTaskTable<int32_t> t = dp_task_table(d_i32, (size_t)n);
    a.b = view(ctx); a.n_tasks = n;
    a.read_idx = t.read; a.rep_start = t.start; a.rep_end = t.end; a.gain = t.gain; a.mism = t.mism; a.indel = t.indel; a.unit_off = t.unit_off;
    { mtr_status s = dp_launch_reset(ctx, a, sc.per_wave, cells, DP_COUNTERS_KEPT); if (s != MTR_OK) return s; }
    hipLaunchKernelGGL(mtr_k_align, dim3((unsigned)sc.waves), dim3(64), 0, ctx->stream, a);
    HIPCHK(hipGetLastError()); return MTR_OK;
}
// what mtr_k_align and mtr_k_scan_offsets left of the report's repeats, for the kernels that print them
static AlignRenderArgs render_args(const mtr_ctx *ctx)
{
    AlignRenderArgs a{};
    const DpTaskTable<int32_t> t = dp_task_table<int32_t>(ctx->d_ra_i32, (size_t)ctx->rep_total);
    a.b = view(ctx); a.n_repeats = (int32_t)ctx->rep_total;
    a.read_idx = t.read; a.rep_start = t.start; a.ops_len = ctx->d_ra_len; a.ends = ctx->d_ra_ends;
    a.path = ctx->d_ra_ops; a.path_off = ctx->d_ra_off; a.rec_of = ctx->d_ra_rec; a.work_counter = ctx->d_work;
    return a;
}
static mtr_status report_alignments(mtr_ctx *ctx)
{
    if (ctx->ra_ready) return MTR_OK;
    { mtr_status st = report_chains(ctx); if (st != MTR_OK) return st; }
    const int n = ctx->n_reads; const int64_t R = ctx->rep_total;
    HIPCHK(ctx->d_ra_coloff.ensure(((size_t)R + 1) * 8));
    if (R == 0) {
        HIPCHK(hipMemsetAsync(ctx->d_ra_coloff, 0, 8, ctx->stream)); HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->ra_columns = 0; ctx->ra_ready = true;
        return MTR_OK;
    }
    if (R > (int64_t)INT32_MAX) { ctx->err = "more reported repeats than one alignment launch takes"; return MTR_ERR_OVERFLOW; }
    read_switches(ctx->sw);
    const RecordView v = record_view(ctx); const ChainView ch = chain_view(ctx);
    HIPCHK(ctx->d_ra_sizes.ensure(MTR_OFFSETS_LEN(n) * 8));
    const AlignSizes z = align_sizes(ctx->d_ra_sizes, n);
    HIPCHK(hipMemsetAsync(z.max_cells, 0, 8, ctx->stream));
    hipLaunchKernelGGL(mtr_k_align_sizes, dim3((unsigned)n), dim3(64), 0, ctx->stream, v, ch, (const int32_t *)ctx->d_lens,
                       z.read_cap, z.read_units, (unsigned long long *)z.max_cells);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mtr_k_scan_offsets<int64_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int64_t *)z.read_cap, (int64_t)n, z.cap_base);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int64_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int64_t *)z.read_units, (int64_t)n, z.unit_base);
    HIPCHK(hipGetLastError());
    int64_t unit_bytes = 0, tail[2] = { 0, 0 };                           // tail: the paths' bytes (cap_base[n]), the largest DP's cells behind them
    HIPCHK(hipMemcpyAsync(&unit_bytes, z.unit_base + n, 8, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(hipMemcpyAsync(tail, z.cap_base + n, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const size_t ops_bytes = (size_t)tail[0], cells = (size_t)std::max<int64_t>(tail[1], 1);
    if (unit_bytes > (int64_t)INT32_MAX) { ctx->err = "the units of the reported repeats exceed 2 GB"; return MTR_ERR_OVERFLOW; }
    DpScratch sc; { mtr_status s = dp_scratch(ctx, dp_matrix_bytes(cells), (int)R, sc); if (s != MTR_OK) return s; }
    DBG("report_alignments: %lld repeats, cells %zu, waves %d, scratch %zu, paths %zu bytes", (long long)R, cells, sc.waves, sc.total, ops_bytes);
    const size_t nt = (size_t)R;
    HIPCHK(ctx->d_ra_i32.ensure(dp_task_ints(nt) * 4)); HIPCHK(ctx->d_ra_len.ensure(nt * 4)); HIPCHK(ctx->d_ra_ends.ensure(nt * 8));
    HIPCHK(ctx->d_ra_units.ensure((size_t)unit_bytes + 16)); HIPCHK(ctx->d_ra_ops.ensure(ops_bytes + 16));
    HIPCHK(ctx->d_ra_off.ensure((nt + 1) * 8)); HIPCHK(ctx->d_ra_rec.ensure(nt * sizeof(void *)));
    const DpTaskTable<int32_t> tab = dp_task_table<int32_t>(ctx->d_ra_i32, nt);
    AlignTaskDst t{};
    t.read_idx = tab.read; t.rep_start = tab.start; t.rep_end = tab.end; t.gain = tab.gain; t.mism = tab.mism; t.indel = tab.indel;
    t.unit_off = tab.unit_off; t.ops_off = ctx->d_ra_off; t.units = ctx->d_ra_units; t.rec_of = ctx->d_ra_rec;
    hipLaunchKernelGGL(mtr_k_align_tasks, dim3((unsigned)n), dim3(64), 0, ctx->stream, v, ch, (const int32_t *)ctx->d_lens,
                       (const int64_t *)z.cap_base, (const int64_t *)z.unit_base, R, t);
    HIPCHK(hipGetLastError());
    AlignArgs a{}; a.units = ctx->d_ra_units; a.ops = ctx->d_ra_ops; a.ops_off = ctx->d_ra_off; a.ops_len = ctx->d_ra_len; a.ends = ctx->d_ra_ends;
    { mtr_status s = launch_align(ctx, a, (int32_t)R, ctx->d_ra_i32, cells, sc); if (s != MTR_OK) return s; }
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)ctx->d_ra_len, R, (int64_t *)ctx->d_ra_coloff);
    HIPCHK(hipGetLastError());
    int64_t columns = 0;
    HIPCHK(copy_sync(ctx, &columns, ctx->d_ra_coloff + R, 8, hipMemcpyDeviceToHost));
    { mtr_status st = check_status(ctx); if (st != MTR_OK) return st; }
    ctx->ra_columns = columns; ctx->ra_ready = true;
    return MTR_OK;
}

extern "C" mtr_status mtr_report_alignments_device(mtr_ctx *ctx, const mtr_report_align_dst *dst, int64_t *out_repeats, int64_t *out_columns)
{
    if (!ctx || !out_repeats || !out_columns) return MTR_ERR_BAD_ARG;
    { mtr_status r = results_ready(ctx, false); if (r != MTR_OK) return r; }
    HIPCHK(hipSetDevice(ctx->device));
    { mtr_status st = report_alignments(ctx); if (st != MTR_OK) return st; }
    const int64_t R = ctx->rep_total, Cn = ctx->ra_columns;
    *out_repeats = R; *out_columns = Cn;
    if (!dst) return MTR_OK;
    if (dst->cap_repeats < R || dst->cap_columns < Cn) {
        ctx->err = "destination holds " + std::to_string(dst->cap_repeats) + " repeats / " + std::to_string(dst->cap_columns) + " columns, " +
                   std::to_string(R) + " / " + std::to_string(Cn) + " needed";
        return MTR_ERR_OVERFLOW;
    }
    if (!dst->col_off || (R > 0 && !dst->first) || (Cn > 0 && (!dst->ops || !dst->text))) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipMemcpyAsync(dst->col_off, ctx->d_ra_coloff, ((size_t)R + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (R > 0) {
        AlignRenderArgs a = render_args(ctx);
        a.col_off = ctx->d_ra_coloff; a.n_columns = Cn;
        a.ops = dst->ops; a.text = dst->text; a.first = dst->first;
        HIPCHK(hipMemsetAsync(ctx->d_work, 0, sizeof(unsigned), ctx->stream));
        const unsigned waves = (unsigned)std::min<int64_t>(R, (int64_t)ctx->n_cu * 16);
        hipLaunchKernelGGL(mtr_k_align_render, dim3(waves), dim3(64), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// the -a alignments of a caller's list of records of the resident batch: the table is staged on the host, one copy takes it up
extern "C" mtr_status mtr_alignments(mtr_ctx *ctx, int32_t n, const int32_t *read_idx, const mtr_record *records,
                                     uint8_t **out_ops, int64_t **out_off, int32_t **out_end)
{
    if (!ctx || n < 0 || (n > 0 && (!read_idx || !records)) || !out_ops || !out_off || !out_end) return MTR_ERR_BAD_ARG;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    { mtr_status w = mtr_wait(ctx); if (w != MTR_OK && w != MTR_ERR_DP_TOO_LARGE) return w; }   // after a DP failure: the reads before it are still printed
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    HostArray<int64_t> off = host_array<int64_t>((size_t)n + 1);
    if (!off) return MTR_ERR_OOM;
    off[0] = 0;
    if (n == 0) { *out_ops = host_array<uint8_t>(1).release(); *out_off = off.release(); *out_end = host_array<int32_t>(2).release(); return MTR_OK; }
    const size_t nt = (size_t)n;
    std::vector<int32_t> h(dp_task_ints(nt));
    const DpTaskTable<int32_t> ht = dp_task_table<int32_t>(h.data(), nt);
    std::vector<uint8_t> units; std::vector<int64_t> cap_off(nt + 1, 0);
    size_t cells = 1;
    for (int t = 0; t < n; t++) {
        const mtr_record &r = records[t];
        const int rd = read_idx[t], U = r.rep_period, rows = r.rep_end - r.rep_start + 1;
        if (rd < 0 || rd >= ctx->n_reads || U <= 0 || U >= MTRC_MAX_PERIOD || rows <= 0 || r.rep_start < 0 || r.rep_end > ctx->lens[(size_t)rd]) {
            ctx->err = "bad alignment task " + std::to_string(t); return MTR_ERR_BAD_ARG;
        }
        ht.read[t] = rd; ht.start[t] = r.rep_start; ht.end[t] = r.rep_end; ht.gain[t] = r.match_gain; ht.mism[t] = r.mismatch_penalty; ht.indel[t] = r.indel_penalty;
        ht.unit_off[t] = (int32_t)units.size();
        for (int j = 0; j < U; j++) { const char ch = r.unit[j]; units.push_back(ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3); }
        // columns = rows + deletions; every deletion costs indel_penalty out of a score of at most match_gain per row
        const size_t max_del = (size_t)std::max(r.match_gain, 1) * (size_t)rows / (size_t)std::max(r.indel_penalty, 1);
        cap_off[(size_t)t + 1] = cap_off[(size_t)t] + (int64_t)(((size_t)rows + max_del + (size_t)U + 64 + 3) & ~(size_t)3);
        cells = std::max(cells, (size_t)rows * (size_t)(U + 1));
    }
    ht.unit_off[n] = (int32_t)units.size();
    DpScratch sc; { mtr_status s = dp_scratch(ctx, dp_matrix_bytes(cells), n, sc); if (s != MTR_OK) return s; }
    const size_t ops_bytes = (size_t)cap_off[nt];
    HIPCHK(ctx->d_al_i32.ensure(h.size() * 4)); HIPCHK(ctx->d_al_len.ensure(nt * 4)); HIPCHK(ctx->d_al_units.ensure(units.size() + 16));
    HIPCHK(ctx->d_al_ops.ensure(ops_bytes + 16)); HIPCHK(ctx->d_al_off.ensure((nt + 1) * 8)); HIPCHK(ctx->d_al_ends.ensure(nt * 8));
    HIPCHK(hipMemcpyAsync(ctx->d_al_i32, h.data(), h.size() * 4, hipMemcpyHostToDevice, ctx->stream)); HIPCHK(hipMemcpyAsync(ctx->d_al_units, units.data(), units.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_al_off, cap_off.data(), (nt + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    AlignArgs a{}; a.units = ctx->d_al_units; a.ops = ctx->d_al_ops; a.ops_off = ctx->d_al_off; a.ops_len = ctx->d_al_len; a.ends = ctx->d_al_ends;
    { mtr_status s = launch_align(ctx, a, n, ctx->d_al_i32, cells, sc); if (s != MTR_OK) return s; }
    std::vector<int32_t> len(nt); std::vector<uint8_t> raw(ops_bytes);
    HostArray<int32_t> ends = host_array<int32_t>(nt * 2);
    if (!ends) return MTR_ERR_OOM;
    HIPCHK(hipMemcpyAsync(ends.get(), ctx->d_al_ends, nt * 8, hipMemcpyDeviceToHost, ctx->stream)); HIPCHK(hipMemcpyAsync(len.data(), ctx->d_al_len, nt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(raw.data(), ctx->d_al_ops, ops_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    { mtr_status st = check_status(ctx); if (st != MTR_OK && !(st == MTR_ERR_DP_TOO_LARGE && ctx->run_status == MTR_ERR_DP_TOO_LARGE)) return st; }
    for (int t = 0; t < n; t++) off[(size_t)t + 1] = off[(size_t)t] + len[(size_t)t];
    HostArray<uint8_t> ops = host_array<uint8_t>((size_t)std::max<int64_t>(off[nt], 1));
    if (!ops) return MTR_ERR_OOM;
    for (int t = 0; t < n; t++) memcpy(ops.get() + off[(size_t)t], raw.data() + cap_off[(size_t)t], (size_t)len[(size_t)t]);
    for (int t = 0; t < n; t++) ends[2 * t] = records[t].rep_start - 1 + ends[2 * t];       // window row -> read position
    *out_ops = ops.release(); *out_off = off.release(); *out_end = ends.release();
    return MTR_OK;
}
