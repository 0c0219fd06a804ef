// motif_host.hip.inc — the hosts of the motif calls, included by mtr_abi.hip below the report's text: the motif catalogue of the report's repeats,
// the known-motif search, and the locus search with the round (loci_round and its buffers) that genotype_host.hip.inc goes through as well.  What
// the sizes and slices are is dp_task_plan.h (DESIGN.md 7i-15); here the buffers, the uploads, the launches and the looks at the device.

// ---- the motif catalogue of the report's repeats (report_motif.hip.inc) -----------------------------------------------------------
// Only the number of groups and of motif bytes come to the host.
// The rows' working arrays in three buffers of the context: d_mo_i32 = rotation | motif_len | read | bases | slot_of | leader | first | lead_len | group,
// d_mo_i64 = hash | copies | unit_off (n + 1) | group_of (n + 1) | len_off (n + 1), d_mo_u8 = strand | the motifs' bytes in the units' layout
struct MotifWork { MotifRows rows; unsigned *slot_of; int32_t *leader, *first, *lead_len, *group; int64_t *group_of, *len_off; };
static mtr_status motif_work(mtr_ctx *ctx, int64_t n, int64_t unit_bytes, MotifWork &w)
{
    const size_t nr = (size_t)n;
    HIPCHK(ctx->d_mo_i32.ensure((9 * nr + 1) * 4)); HIPCHK(ctx->d_mo_i64.ensure((5 * nr + 3) * 8)); HIPCHK(ctx->d_mo_u8.ensure(nr + (size_t)unit_bytes + 16));
    int32_t *i = ctx->d_mo_i32; int64_t *l = ctx->d_mo_i64; uint8_t *b = ctx->d_mo_u8;
    w.rows.rotation = i; w.rows.motif_len = i + nr; w.rows.read = i + 2 * nr; w.rows.bases = i + 3 * nr;
    w.slot_of = (unsigned *)(i + 4 * nr); w.leader = i + 5 * nr; w.first = i + 6 * nr; w.lead_len = i + 7 * nr; w.group = i + 8 * nr;
    w.rows.hash = (unsigned long long *)l; w.rows.copies = l + nr; w.rows.unit_off = l + 2 * nr; w.group_of = l + 3 * nr + 1; w.len_off = l + 4 * nr + 2;
    w.rows.strand = b; w.rows.motif = b + nr;
    return MTR_OK;
}
// the columns per group in d_mo_g32 = first | repeats | reads, d_mo_g64 = motif_off (G + 1) | copies | bases, and d_mo_motifs
static MotifGroups motif_groups(const mtr_ctx *ctx, const MotifWork &w)
{
    const size_t G = (size_t)ctx->mo_groups;
    int32_t *i = ctx->d_mo_g32; int64_t *l = ctx->d_mo_g64;
    return { w.group, l, ctx->d_mo_motifs, i, i + G, i + 2 * G, l + G + 1, l + 2 * G + 1 };
}
// The rows are in place (mtr_k_unit_motif or mtr_k_unit_motif_rows is enqueued): group them.  table_slots: 0 = twice the rows, rounded up to a
// power of two; else the caller's power of two above n (mtr_test_unit_motifs).  Leaves mo_groups / mo_motif_bytes and the stream synchronised.
static mtr_status motif_group(mtr_ctx *ctx, int64_t n, int64_t table_slots, const MotifWork &w)
{
    ctx->mo_groups = 0; ctx->mo_motif_bytes = 0;
    if (n == 0) {
        HIPCHK(ctx->d_mo_g64.ensure(8));
        HIPCHK(hipMemsetAsync(ctx->d_mo_g64, 0, 8, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return MTR_OK;
    }
    int64_t slots = table_slots;
    if (slots == 0) for (slots = 64; slots < 2 * n; slots <<= 1) { }
    HIPCHK(ctx->d_mo_table.ensure((size_t)slots * 4));
    HIPCHK(hipMemsetAsync(ctx->d_mo_table, 0xff, (size_t)slots * 4, ctx->stream));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(mtr_k_motif_insert, dim3(blocks), dim3(256), 0, ctx->stream, (int32_t)n, w.rows, (unsigned *)ctx->d_mo_table, (unsigned)(slots - 1), w.slot_of);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mtr_k_motif_leader, dim3(blocks), dim3(256), 0, ctx->stream, (int32_t)n, (const int32_t *)w.rows.motif_len, (const unsigned *)ctx->d_mo_table,
                       (const unsigned *)w.slot_of, w.leader, w.first, w.lead_len);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)w.first, n, w.group_of);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)w.lead_len, n, w.len_off);
    HIPCHK(hipGetLastError());
    int64_t G = 0, M = 0;
    HIPCHK(hipMemcpyAsync(&G, w.group_of + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&M, w.len_off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (G < 1 || G > n || M < 0) { ctx->err = "the motif table is inconsistent"; return MTR_ERR_HIP; }
    ctx->mo_groups = G; ctx->mo_motif_bytes = M;
    const size_t g = (size_t)G;
    HIPCHK(ctx->d_mo_g32.ensure(3 * g * 4)); HIPCHK(ctx->d_mo_g64.ensure((3 * g + 1) * 8)); HIPCHK(ctx->d_mo_motifs.ensure((size_t)M + 16));
    const MotifGroups mg = motif_groups(ctx, w);
    HIPCHK(hipMemsetAsync(mg.repeats, 0, 2 * g * 4, ctx->stream));             // repeats | reads
    HIPCHK(hipMemsetAsync(mg.copies, 0, 2 * g * 8, ctx->stream));              // copies | bases
    hipLaunchKernelGGL(mtr_k_motif_groups, dim3(blocks), dim3(256), 0, ctx->stream, (int32_t)n, w.rows, (const int32_t *)w.leader, (const int64_t *)w.group_of,
                       (const int64_t *)w.len_off, mg);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

static mtr_status report_motifs(mtr_ctx *ctx)
{
    if (ctx->mo_ready) return MTR_OK;
    { mtr_status st = report_chains(ctx); if (st != MTR_OK) return st; }
    const int64_t R = ctx->rep_total;
    if (R > (int64_t)INT32_MAX / 2) { ctx->err = "more reported repeats than the motif table takes"; return MTR_ERR_OVERFLOW; }
    MotifWork w{};
    { mtr_status st = motif_work(ctx, R, ctx->rep_unit_bytes, w); if (st != MTR_OK) return st; }
    if (R > 0) {
        const int n = ctx->n_reads;
        hipLaunchKernelGGL(mtr_k_unit_motif, dim3((unsigned)n), dim3(64), 0, ctx->stream, record_view(ctx), chain_view(ctx),
                           (const int64_t *)chain_offsets(ctx->d_ch_off, n).unit_base, R, ctx->rep_unit_bytes, w.rows);
        HIPCHK(hipGetLastError());
    }
    { mtr_status st = motif_group(ctx, R, 0, w); if (st != MTR_OK) return st; }
    ctx->mo_ready = true;
    return MTR_OK;
}

extern "C" mtr_status mtr_report_motifs_device(mtr_ctx *ctx, const mtr_report_motif_dst *dst, int64_t *out_repeats, int64_t *out_groups, int64_t *out_motif_bytes)
{
    if (!ctx || !out_repeats || !out_groups || !out_motif_bytes) return MTR_ERR_BAD_ARG;
    { mtr_status r = results_ready(ctx, false); if (r != MTR_OK) return r; }
    HIPCHK(hipSetDevice(ctx->device));
    { mtr_status st = report_motifs(ctx); if (st != MTR_OK) return st; }
    const int64_t R = ctx->rep_total, G = ctx->mo_groups, M = ctx->mo_motif_bytes;
    *out_repeats = R; *out_groups = G; *out_motif_bytes = M;
    if (!dst) return MTR_OK;
    if (dst->cap_repeats < R || dst->cap_groups < G || dst->cap_motif_bytes < M) {
        ctx->err = "destination holds " + std::to_string(dst->cap_repeats) + " repeats / " + std::to_string(dst->cap_groups) + " groups / " +
                   std::to_string(dst->cap_motif_bytes) + " motif bytes, " + std::to_string(R) + " / " + std::to_string(G) + " / " + std::to_string(M) + " needed";
        return MTR_ERR_OVERFLOW;
    }
    if (!dst->motif_off || (R > 0 && (!dst->strand || !dst->rotation || !dst->motif_len || !dst->group)) || (M > 0 && !dst->motifs) ||
        (G > 0 && (!dst->g_first || !dst->g_repeats || !dst->g_reads || !dst->g_copies || !dst->g_bases))) {
        ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG;
    }
    MotifWork w{};
    { mtr_status st = motif_work(ctx, R, ctx->rep_unit_bytes, w); if (st != MTR_OK) return st; }      // (the buffers are there: the layout alone)
    const MotifGroups mg = motif_groups(ctx, w);
    const size_t r = (size_t)R, g = (size_t)G;
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    HIPCHK(hipMemcpyAsync(dst->motif_off, mg.motif_off, (g + 1) * 8, dd, ctx->stream));
    if (R > 0) {
        HIPCHK(hipMemcpyAsync(dst->strand, w.rows.strand, r, dd, ctx->stream)); HIPCHK(hipMemcpyAsync(dst->rotation, w.rows.rotation, r * 4, dd, ctx->stream));
        HIPCHK(hipMemcpyAsync(dst->motif_len, w.rows.motif_len, r * 4, dd, ctx->stream)); HIPCHK(hipMemcpyAsync(dst->group, mg.group, r * 4, dd, ctx->stream));
    }
    if (M > 0) HIPCHK(hipMemcpyAsync(dst->motifs, mg.motifs, (size_t)M, dd, ctx->stream));
    if (G > 0) {
        HIPCHK(hipMemcpyAsync(dst->g_first, mg.first, g * 4, dd, ctx->stream)); HIPCHK(hipMemcpyAsync(dst->g_repeats, mg.repeats, g * 4, dd, ctx->stream));
        HIPCHK(hipMemcpyAsync(dst->g_reads, mg.reads, g * 4, dd, ctx->stream)); HIPCHK(hipMemcpyAsync(dst->g_copies, mg.copies, g * 8, dd, ctx->stream));
        HIPCHK(hipMemcpyAsync(dst->g_bases, mg.bases, g * 8, dd, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- known-motif search (motif_search.hip.inc) -------------------------------------------------------------------------------------
// Only the lengths (already on the host) decide the work: one argsort per call, the slots' tables and at most five work lists go up, nothing
// comes back but the status word.  Nothing kept lives in d_scratch (every user sizes and fills it per launch), so growing it here is safe.
// (the checks in two parts: the locus search has arguments of its own to refuse between them; the scores', the total's and a motif's own
// checks and words are loci_args.h's, which the genotype calls reach for their loci's motifs too)
static mtr_status search_motifs_check_args(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, int32_t n_motifs, int32_t gain, int32_t mismatch, int32_t indel)
{
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    if (n_motifs <= 0) { ctx->err = "n_motifs = " + std::to_string(n_motifs) + ": at least one motif is needed"; return MTR_ERR_BAD_ARG; }
    if (!motifs || !motif_off) { ctx->err = "motifs or motif_off is NULL"; return MTR_ERR_BAD_ARG; }
    if (!la_check_scores(gain, mismatch, indel, ctx->err)) return MTR_ERR_BAD_ARG;
    if (!la_check_motif_total(n_motifs, motif_off[n_motifs] - motif_off[0], ctx->err)) return MTR_ERR_BAD_ARG;
    for (int32_t m = 0; m < n_motifs; m++) {
        const char *s = motifs + motif_off[m];
        const int64_t U = motif_off[m + 1] - motif_off[m];
        if (U < 0) { ctx->err = "motif_off decreases at motif " + std::to_string(m); return MTR_ERR_BAD_ARG; }
        const int64_t t = la_seq_check(false, s, U);
        if (t < U) { ctx->err = la_refusal(la_motif_name(m), false, t, s, U); return MTR_ERR_BAD_ARG; }
    }
    return la_check_hits(ctx->n_reads, n_motifs, ctx->err) ? MTR_OK : MTR_ERR_BAD_ARG;
}
// the reference's WrapDPsize test (wrap_around_DP.c:260) for the longest read first, then for the read it names
static mtr_status search_motifs_check_size(mtr_ctx *ctx, const int64_t *motif_off, int32_t n_motifs)
{
    for (int32_t m = 0; m < n_motifs; m++) {
        const long long U = motif_off[m + 1] - motif_off[m];
        if ((U + 1) * (long long)ctx->Lmax + U < ctx->wrap_dp_size) continue;
        for (int i = 0; i < ctx->n_reads; i++)
            if ((U + 1) * (long long)ctx->lens[(size_t)i] + U >= ctx->wrap_dp_size) {
                ctx->err = "You need to increse the value of WrapDPsize. (read " + std::to_string(i) + " of " + std::to_string(ctx->lens[(size_t)i]) + " bases against motif " +
                           std::to_string(m) + " of " + std::to_string(U) + " bases exceeds " + std::to_string(ctx->wrap_dp_size) + " cells)";
                return MTR_ERR_DP_TOO_LARGE;
            }
    }
    return MTR_OK;
}

// What motif_slots makes of the motifs' text, and its way to the device: unit_off (S + 1) where the caller has room for it, bits (S) at the front of
// their buffer, the codes (+ 16: the kernels' dword loads read past the last) in a buffer of their own.  A prepared catalogue's tables, built on the device, never come here.
// ls: the lane slots too, behind unit_off as a round's i32 has them; the locus search sends them between the offsets and the bits.
struct SlotTables { std::vector<uint8_t> units; std::vector<int32_t> unit_off; std::vector<uint64_t> bits; };
static mtr_status upload_lane_slots(mtr_ctx *ctx, const LaneSlots &ls, int32_t *d_slot_q, int32_t *d_q_slot)
{
    HIPCHK(copy_sync(ctx, d_slot_q, ls.slot_q.data(), ls.slot_q.size() * 4, hipMemcpyHostToDevice));
    if (!ls.q_slot.empty()) HIPCHK(copy_sync(ctx, d_q_slot, ls.q_slot.data(), ls.q_slot.size() * 4, hipMemcpyHostToDevice));
    return MTR_OK;
}
static mtr_status upload_slot_tables(mtr_ctx *ctx, const SlotTables &t, int32_t *d_uoff, DevBuf<int64_t> &d_bits, DevBuf<uint8_t> &d_units, const LaneSlots *ls = nullptr)
{
    const LociRoundLayout at = loci_slot_layout(t.bits.size());
    HIPCHK(d_bits.ensure(at.i64_bytes)); HIPCHK(d_units.ensure(t.units.size() + 16));      // (the search's bits lead a larger buffer, sized before)
    HIPCHK(copy_sync(ctx, d_uoff, t.unit_off.data(), t.unit_off.size() * 4, hipMemcpyHostToDevice));
    if (ls) { mtr_status st = upload_lane_slots(ctx, *ls, d_uoff + at.slot_q, d_uoff + at.q_slot); if (st != MTR_OK) return st; }
    HIPCHK(copy_sync(ctx, d_bits, t.bits.data(), t.bits.size() * 8, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_units, t.units.data(), t.units.size(), hipMemcpyHostToDevice));
    return MTR_OK;
}

extern "C" mtr_status mtr_search_motifs_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, int32_t n_motifs, int32_t gain, int32_t mismatch,
                                               int32_t indel, int32_t both_strands, const mtr_motif_hits_dst *dst, int64_t *out_hits)
{
    if (!ctx || !out_hits) return MTR_ERR_BAD_ARG;
    *out_hits = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    { mtr_status st = search_motifs_check_args(ctx, motifs, motif_off, n_motifs, gain, mismatch, indel); if (st != MTR_OK) return st; }
    { mtr_status st = search_motifs_check_size(ctx, motif_off, n_motifs); if (st != MTR_OK) return st; }
    const int n = ctx->n_reads;
    const int64_t H = (int64_t)n * n_motifs;
    *out_hits = H;
    if (!dst) return MTR_OK;
    if (dst->cap_hits < H) { ctx->err = "destination holds " + std::to_string(dst->cap_hits) + " hits, " + std::to_string(H) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->fields || !dst->score || !dst->ratio || !dst->strand) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    const int lane_max = ctx->sw.motif_lane_max, lane_rows = ctx->sw.motif_lane_rows;
    const int ns = both_strands ? 2 : 1, S = n_motifs * ns;
    // the reads by descending length (ties in input order), the first n_long of them beyond the lane path
    std::vector<int32_t> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return ctx->lens[(size_t)x] > ctx->lens[(size_t)y]; });
    int n_long = 0;
    while (n_long < n && ctx->lens[(size_t)order[(size_t)n_long]] > lane_rows) n_long++;
    const long long L_first = ctx->lens[(size_t)order[0]], L_lane = n_long < n ? ctx->lens[(size_t)order[(size_t)n_long]] : 0;
    SlotTables t;
    motif_slots(motifs, motif_off, n_motifs, ns, t.units, t.unit_off, t.bits);
    // the work lists: one per bucket of the lane path (groups of 64 reads of the order from n_long on), one of the wave path (reads)
    enum { N_LISTS = DP_LAUNCHES };
    std::vector<int32_t> l_slot[N_LISTS]; std::vector<int64_t> l_first[N_LISTS]; int l_umax[N_LISTS] = { 0, 0, 0, 0, 0 };
    const int64_t groups = ((int64_t)(n - n_long) + 63) / 64;
    for (int k = 0; k < N_LISTS; k++) l_first[k].push_back(0);
    for (int slot = 0; slot < S; slot++) {
        const int U = t.unit_off[(size_t)slot + 1] - t.unit_off[(size_t)slot];
        const bool lane = U <= lane_max && groups > 0;
        if (lane) {
            int k = 0; while (dp_bucket_ub(k) < U) k++;
            l_slot[k].push_back(slot); l_first[k].push_back(l_first[k].back() + groups); l_umax[k] = std::max(l_umax[k], U);
        }
        const int64_t by_wave = U <= lane_max ? n_long : n;
        if (by_wave > 0) { l_slot[4].push_back(slot); l_first[4].push_back(l_first[4].back() + by_wave); l_umax[4] = std::max(l_umax[4], U); }
    }
    // device copies: d_ms_i32 = order | unit_off | the lists' slots, d_ms_i64 = bits | the lists' firsts
    const size_t nr = (size_t)n, sS = (size_t)S;
    HIPCHK(ctx->d_ms_i32.ensure((nr + sS + 1 + N_LISTS * sS) * 4)); HIPCHK(ctx->d_ms_i64.ensure((sS + N_LISTS * (sS + 1)) * 8));
    HIPCHK(ctx->d_ms_res.ensure((size_t)H * (size_t)ns * MS_RES * 4)); HIPCHK(ctx->d_ms_status.ensure(4)); HIPCHK(ctx->d_ms_counter.ensure(N_LISTS * 8));
    int32_t *d_order = ctx->d_ms_i32, *d_uoff = d_order + nr, *d_slots = d_uoff + sS + 1;
    int64_t *d_bits = ctx->d_ms_i64, *d_firsts = d_bits + sS;
    HIPCHK(copy_sync(ctx, d_order, order.data(), nr * 4, hipMemcpyHostToDevice));
    { mtr_status st = upload_slot_tables(ctx, t, d_uoff, ctx->d_ms_i64, ctx->d_ms_units); if (st != MTR_OK) return st; }
    for (int k = 0; k < N_LISTS; k++) {
        if (l_slot[k].empty()) continue;
        HIPCHK(copy_sync(ctx, d_slots + (size_t)k * sS, l_slot[k].data(), l_slot[k].size() * 4, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, d_firsts + (size_t)k * (sS + 1), l_first[k].data(), l_first[k].size() * 8, hipMemcpyHostToDevice));
    }
    // the launches' wavefronts and scratch (dp_task_plan.h: the five-launch plan)
    const int64_t l_items[N_LISTS] = { l_first[0].back(), l_first[1].back(), l_first[2].back(), l_first[3].back(), l_first[4].back() };
    const DpLaunchPlan plan = dp_search_plan(L_lane, L_first, l_umax, l_items, DpPick{ ctx });
    { mtr_status s = ensure_scratch(ctx, plan.scratch); if (s != MTR_OK) return s; }
    HIPCHK(hipMemsetAsync(ctx->d_ms_status, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_ms_counter, 0, N_LISTS * 8, ctx->stream));
    MotifSearchArgs a{};
    a.b.packed = ctx->d_packed; a.b.woff = ctx->d_woff; a.b.lens = ctx->d_lens; a.b.order = d_order; a.b.n_reads = n;
    a.order = d_order; a.n_reads = n; a.n_long = n_long; a.units = ctx->d_ms_units; a.unit_off = d_uoff; a.bits = (const uint64_t *)d_bits;
    a.n_motifs = n_motifs; a.n_strands = ns; a.G = gain; a.MM = mismatch; a.D = indel; a.res = ctx->d_ms_res;
    a.scratch = ctx->d_scratch; a.status = ctx->d_ms_status; a.dp16_max_rows = ctx->sw.dp16_max_rows;
    const mtr_status launched = dp_plan_launches(ctx, plan, a, (unsigned long long *)ctx->d_ms_counter, [&](int k, dim3 grid, dim3 block) {
        a.work = { d_slots + (size_t)k * sS, d_firsts + (size_t)k * (sS + 1), (int32_t)l_slot[k].size(), l_first[k].back() };
        DBG("search_motifs: list %d: %zu slots, %lld items, %d wavefronts of %zu bytes", k, l_slot[k].size(), (long long)l_first[k].back(), plan.waves[k], plan.per_wave[k]);
        if (k < DP_LANE_BUCKETS) LAUNCH_BY_BUCKET(mtr_k_motif_lanes, dp_bucket_ub(k), grid, block, ctx->stream, a);
        else hipLaunchKernelGGL(mtr_k_motif_waves, grid, block, 0, ctx->stream, a);
    });
    if (launched != MTR_OK) return launched;
    // the status before the columns: a failed search writes nothing
    int32_t dev = 0;
    HIPCHK(copy_sync(ctx, &dev, ctx->d_ms_status, 4, hipMemcpyDeviceToHost));
    if (dev == DEV_ERR_DP_TOO_LARGE) { ctx->err = "You need to increse the value of WrapDPsize. (a DP of the motif search exceeded it or its scratch)"; return MTR_ERR_DP_TOO_LARGE; }
    if (dev != DEV_OK) { ctx->err = "the motif search failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    const MotifHitsOut out = { dst->fields, dst->score, dst->ratio, dst->strand };
    hipLaunchKernelGGL(mtr_k_motif_pack, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t *)ctx->d_ms_res, (int32_t)ns, H, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- known-motif locus search (motif_loci.hip.inc) ---------------------------------------------------------------------------------
// Round by round: the host knows how many intervals a round has and their longest (LOCI_STATE, one small copy per round), sizes the round's
// arrays and scratch from that, and enqueues its kernels; everything else - the bins, the work lists, the hits, the children - is made on the device.
// at least `bytes`, with what the first `keep` bytes hold (the hit list grows from round to round)
template <typename T>
static hipError_t grow_keeping(mtr_ctx *ctx, DevBuf<T> &b, size_t keep, size_t bytes)
{
    if (b.p && bytes <= b.cap) return hipSuccess;
    T *fresh = nullptr;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 256);
    hipError_t e = hipMalloc((void **)&fresh, want);
    if (e != hipSuccess) return e;
    if (keep > 0 && b.p) e = copy_sync(ctx, fresh, b.p, keep, hipMemcpyDeviceToDevice);
    b.release();
    b.p = fresh; b.cap = want;
    return e;
}

// A round's buffers at least as large as dp_task_plan.h's layout of (S, nq, nt) says, and of `a` what both hosts set alike: the batch, the switches,
// and every slice of b but the slots' tables (unit_off | bits | units: the caller's, or a prepared catalogue's).  nt = 0, the locus search before
// its first round: no task array yet.
static mtr_status loci_round_bufs(mtr_ctx *ctx, LociRoundBufs &b, size_t S, size_t nq, size_t nt, LociArgs &a)
{
    LociRoundLayout l;
    if (!loci_round_layout(S, nq, nt, l, ctx->err)) return MTR_ERR_OVERFLOW;
    HIPCHK(b.i32.ensure(l.i32_bytes)); HIPCHK(b.bin32.ensure(l.bin32_bytes)); HIPCHK(b.bin64.ensure(l.bin64_bytes)); HIPCHK(b.state.ensure(l.state_bytes)); HIPCHK(b.counter.ensure(l.counter_bytes));
    if (nt > 0) { HIPCHK(b.task32.ensure(l.task32_bytes)); HIPCHK(b.res.ensure(l.res_bytes)); }
    a.b.packed = ctx->d_packed; a.b.woff = ctx->d_woff; a.b.lens = ctx->d_lens; a.b.order = nullptr; a.b.n_reads = ctx->n_reads;
    a.lane_rows = ctx->sw.motif_lane_rows; a.dp16_max_rows = ctx->sw.dp16_max_rows;
    a.slot_q = b.i32 + l.slot_q; a.q_slot = b.i32 + l.q_slot;
    a.hist = b.bin32; a.groups = a.hist + l.groups; a.tfirst = b.bin64; a.gfirst = a.tfirst + l.gfirst; a.n_bins = (int32_t)l.nb;
    a.tbin = b.task32; a.trank = a.tbin + l.trank; a.sorted = a.tbin + l.sorted; a.wlist = a.tbin + l.wlist; a.res = b.res;
    a.state = b.state;
    return MTR_OK;
}
// A round's one look at the device: the state words, and the verdict in the caller's words (who: "locus search" / "genotype", failed: what failed, where: ", round 3")
static mtr_status loci_round_status(mtr_ctx *ctx, const LociRoundBufs &b, int32_t (&st)[LOCI_STATE], const char *who, const char *failed, const std::string &where)
{
    HIPCHK(copy_sync(ctx, st, b.state, sizeof st, hipMemcpyDeviceToHost));
    if (st[LOCI_STATUS] == DEV_ERR_DP_TOO_LARGE) { ctx->err = std::string("You need to increse the value of WrapDPsize. (a DP of the ") + who + " exceeded it or its scratch)"; return MTR_ERR_DP_TOO_LARGE; }
    if (st[LOCI_STATUS] != DEV_OK) { ctx->err = std::string("the ") + failed + " failed on the device (status " + std::to_string(st[LOCI_STATUS]) + where + ")"; return MTR_ERR_HIP; }
    return MTR_OK;
}

// One round's alignments: `tasks` tasks over a.iv (a.n_iv intervals of at most max_len bases), everything of `a` set but what one launch has of
// its own.  Plans the launches as the search does, bins the tasks, enqueues the up to five DP launches.  counters: five item counters.  who: for MTR_DEBUG.
static mtr_status loci_round(mtr_ctx *ctx, LociArgs &a, const LaneSlots &ls, int64_t tasks, int max_len, unsigned long long *counters, const char *who, int round)
{
    const size_t nb = (size_t)a.n_bins, nt = (size_t)tasks;
    const DpLaunchPlan plan = dp_loci_plan(ls, tasks, max_len, a.lane_rows, DpPick{ ctx });
    { mtr_status s = ensure_scratch(ctx, plan.scratch); if (s != MTR_OK) return s; }
    a.scratch = ctx->d_scratch;
    if (nb > 0) HIPCHK(hipMemsetAsync(a.hist, 0, nb * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(counters, 0, 5 * 8, ctx->stream));
    const dim3 per_task((unsigned)((nt + 255) / 256)), b256(256);
    hipLaunchKernelGGL(mtr_k_loci_bin, per_task, b256, 0, ctx->stream, a);
    if (nb > 0) {
        hipLaunchKernelGGL(mtr_k_loci_groups, dim3((unsigned)((nb + 255) / 256)), b256, 0, ctx->stream, (const int32_t *)a.hist, (int32_t)nb, a.groups);
        hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)a.hist, (int64_t)nb, a.tfirst);
        hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)a.groups, (int64_t)nb, a.gfirst);
        hipLaunchKernelGGL(mtr_k_loci_scatter, per_task, b256, 0, ctx->stream, a);
    }
    HIPCHK(hipGetLastError());
    return dp_plan_launches(ctx, plan, a, counters, [&](int k, dim3 grid, dim3 block) {
        if (k < DP_LANE_BUCKETS) { a.bin0 = ls.q_first[k] * MLO_N_CLASSES; a.bin1 = ls.q_first[k + 1] * MLO_N_CLASSES; }
        DBG("%s: round %d, %lld intervals of at most %d bases, launch %d: %d wavefronts of %zu bytes", who, round, (long long)a.n_iv, max_len, k, plan.waves[k], plan.per_wave[k]);
        if (k < DP_LANE_BUCKETS) LAUNCH_BY_BUCKET(mtr_k_motif_loci_lanes, dp_bucket_ub(k), grid, block, ctx->stream, a);
        else hipLaunchKernelGGL(mtr_k_motif_loci_waves, grid, block, 0, ctx->stream, a);
    });
}

extern "C" mtr_status mtr_search_motif_loci_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, int32_t n_motifs, int32_t gain, int32_t mismatch,
                                                   int32_t indel, int32_t both_strands, int32_t min_score, int32_t max_rounds, int64_t *out_pairs, int64_t *out_loci)
{
    if (!ctx || !out_pairs || !out_loci) return MTR_ERR_BAD_ARG;
    *out_pairs = 0; *out_loci = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    ctx->ml_ready = false;                                                                             // whatever happens below, the loci kept before this call are gone
    { mtr_status st = search_motifs_check_args(ctx, motifs, motif_off, n_motifs, gain, mismatch, indel); if (st != MTR_OK) return st; }
    if (min_score < 1) { ctx->err = "min_score = " + std::to_string(min_score) + ": at least 1"; return MTR_ERR_BAD_ARG; }
    if (max_rounds < 1 || max_rounds > MLO_MAX_ROUNDS) { ctx->err = "max_rounds = " + std::to_string(max_rounds) + " outside 1.." + std::to_string(MLO_MAX_ROUNDS); return MTR_ERR_BAD_ARG; }
    { mtr_status st = search_motifs_check_size(ctx, motif_off, n_motifs); if (st != MTR_OK) return st; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    const int n = ctx->n_reads, ns = both_strands ? 2 : 1, S = n_motifs * ns, minlen = mlo_minlen(min_score, gain);
    const int64_t P = (int64_t)n * n_motifs;
    SlotTables t;
    motif_slots(motifs, motif_off, n_motifs, ns, t.units, t.unit_off, t.bits);
    const LaneSlots ls = lane_slots(t.unit_off, S, ctx->sw.motif_lane_max);
    LociRoundBufs &ml = ctx->ml;
    LociArgs a{};
    { mtr_status s = loci_round_bufs(ctx, ml, (size_t)S, ls.q_slot.size(), 0, a); if (s != MTR_OK) return s; }
    HIPCHK(ctx->d_ml_open.ensure((size_t)P));
    { mtr_status s = upload_slot_tables(ctx, t, ml.i32, ml.i64, ml.units, &ls); if (s != MTR_OK) return s; }
    HIPCHK(hipMemsetAsync(ml.state, 0, LOCI_STATE * 4, ctx->stream)); HIPCHK(hipMemsetAsync(ctx->d_ml_open, 0, (size_t)P, ctx->stream));
    a.n_motifs = n_motifs; a.n_strands = ns; a.G = gain; a.MM = mismatch; a.D = indel;
    a.units = ml.units; a.unit_off = ml.i32; a.bits = (const uint64_t *)(int64_t *)ml.i64;
    // round 0: every pair's whole read
    HIPCHK(ctx->d_ml_iv[0].ensure((size_t)P * sizeof(LociIv)));
    hipLaunchKernelGGL(mtr_k_loci_init, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t *)ctx->d_lens, n_motifs, (int32_t)P, (LociIv *)ctx->d_ml_iv[0]);
    HIPCHK(hipGetLastError());
    int64_t N = P, T = 0;
    int max_len = ctx->Lmax;
    for (int d = 0; d < max_rounds && N > 0; d++) {
        const int64_t tasks = N * ns;
        if (tasks > (int64_t)INT32_MAX || T + N > (int64_t)INT32_MAX) {
            ctx->err = "round " + std::to_string(d) + ": " + std::to_string(tasks) + " alignments after " + std::to_string(T) + " loci are more than 2^31 - 1"; return MTR_ERR_OVERFLOW;
        }
        LociIv *next = nullptr;
        {   // the round's task arrays; the next round holds at most two intervals per interval, the hit list one more hit
            DevBuf<LociIv> &nx = ctx->d_ml_iv[(d + 1) & 1];
            { mtr_status s = loci_round_bufs(ctx, ml, (size_t)S, ls.q_slot.size(), (size_t)tasks, a); if (s != MTR_OK) return s; }
            HIPCHK(nx.ensure(2 * (size_t)N * sizeof(LociIv)));
            HIPCHK(grow_keeping(ctx, ctx->d_ml_hits, (size_t)T * LOCI_HIT * 4, (size_t)(T + N) * LOCI_HIT * 4));
            next = nx;
        }
        a.iv = ctx->d_ml_iv[d & 1]; a.n_iv = (int32_t)N;
        HIPCHK(hipMemsetAsync(a.state + LOCI_NEXT, 0, (LOCI_STATE - LOCI_NEXT) * 4, ctx->stream));
        { mtr_status s = loci_round(ctx, a, ls, tasks, max_len, (unsigned long long *)ml.counter, "search_motif_loci", d); if (s != MTR_OK) return s; }
        const dim3 b256(256);
        hipLaunchKernelGGL(mtr_k_loci_split, dim3((unsigned)((N + 255) / 256)), b256, 0, ctx->stream, a, min_score, (int32_t)minlen, max_rounds, (int32_t)d,
                           next, (int32_t)std::min<int64_t>(2 * N, INT32_MAX), (int32_t *)ctx->d_ml_hits, (int32_t)(T + N), (uint8_t *)ctx->d_ml_open);
        HIPCHK(hipGetLastError());
        // the round's one look at the device: its verdict, the loci so far, the next round's intervals and their longest
        int32_t st[LOCI_STATE];
        { mtr_status s = loci_round_status(ctx, ml, st, "locus search", "locus search", ", round " + std::to_string(d)); if (s != MTR_OK) return s; }
        if (st[LOCI_HITS] < T || st[LOCI_HITS] > T + N || st[LOCI_NEXT] < 0 || st[LOCI_NEXT] > 2 * N || st[LOCI_MAXLEN] > max_len) { ctx->err = "the locus search's lists are inconsistent"; return MTR_ERR_HIP; }
        T = st[LOCI_HITS]; N = st[LOCI_NEXT]; max_len = st[LOCI_MAXLEN];
    }
    // the finish: per pair its loci counted, the offsets, every locus at its rank by start
    const size_t np = (size_t)P, nl = std::max<size_t>((size_t)T, 1);
    HIPCHK(ctx->d_ml_count.ensure(np * 4)); HIPCHK(ctx->d_ml_off.ensure((np + 1) * 8)); HIPCHK(ctx->d_ml_starts.ensure(nl * 4));
    HIPCHK(ctx->d_ml_fields.ensure(nl * 32)); HIPCHK(ctx->d_ml_score.ensure(nl * 4)); HIPCHK(ctx->d_ml_ratio.ensure(nl * 4)); HIPCHK(ctx->d_ml_strand.ensure(nl));
    HIPCHK(hipMemsetAsync(ctx->d_ml_count, 0, np * 4, ctx->stream));
    const dim3 per_hit((unsigned)((nl + 255) / 256)), b256(256);
    if (T > 0) hipLaunchKernelGGL(mtr_k_loci_count, per_hit, b256, 0, ctx->stream, (int32_t *)ctx->d_ml_hits, (int32_t)T, (int32_t *)ctx->d_ml_count);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, dim3(1), dim3(1024), 0, ctx->stream, (const int32_t *)ctx->d_ml_count, P, (int64_t *)ctx->d_ml_off);
    if (T > 0) {
        const MotifLociOut out = { ctx->d_ml_fields, ctx->d_ml_score, ctx->d_ml_ratio, ctx->d_ml_strand };
        hipLaunchKernelGGL(mtr_k_loci_starts, per_hit, b256, 0, ctx->stream, (const int32_t *)ctx->d_ml_hits, (int32_t)T, (const int64_t *)ctx->d_ml_off, (int32_t *)ctx->d_ml_starts);
        hipLaunchKernelGGL(mtr_k_loci_place, per_hit, b256, 0, ctx->stream, (const int32_t *)ctx->d_ml_hits, (int32_t)T, (const int64_t *)ctx->d_ml_off,
                           (const int32_t *)ctx->d_ml_starts, out);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->ml_ready = true; ctx->ml_pairs = P; ctx->ml_loci = T;
    *out_pairs = P; *out_loci = T;
    return MTR_OK;
}

extern "C" mtr_status mtr_motif_loci_copy_device(mtr_ctx *ctx, const mtr_motif_loci_dst *dst)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (!ctx->ml_ready) { ctx->err = "no loci kept: mtr_search_motif_loci_device comes first (an upload discards what it kept)"; return MTR_ERR_BAD_ARG; }
    if (!dst) { ctx->err = "dst is NULL"; return MTR_ERR_BAD_ARG; }
    const int64_t P = ctx->ml_pairs, T = ctx->ml_loci;
    if (dst->cap_pairs < P || dst->cap_loci < T) {
        ctx->err = "destination holds " + std::to_string(dst->cap_pairs) + " pairs and " + std::to_string(dst->cap_loci) + " loci, " + std::to_string(P) + " and " + std::to_string(T) + " needed";
        return MTR_ERR_OVERFLOW;
    }
    if (!dst->loci_off || !dst->open || (T > 0 && (!dst->fields || !dst->score || !dst->ratio || !dst->strand))) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    const size_t p = (size_t)P, t = (size_t)T;
    HIPCHK(hipMemcpyAsync(dst->loci_off, ctx->d_ml_off, (p + 1) * 8, dd, ctx->stream)); HIPCHK(hipMemcpyAsync(dst->open, ctx->d_ml_open, p, dd, ctx->stream));
    if (T > 0) {
        HIPCHK(hipMemcpyAsync(dst->fields, ctx->d_ml_fields, t * 32, dd, ctx->stream)); HIPCHK(hipMemcpyAsync(dst->score, ctx->d_ml_score, t * 4, dd, ctx->stream));
        HIPCHK(hipMemcpyAsync(dst->ratio, ctx->d_ml_ratio, t * 4, dd, ctx->stream)); HIPCHK(hipMemcpyAsync(dst->strand, ctx->d_ml_strand, t, dd, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}
