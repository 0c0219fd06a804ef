// genotype_host.hip.inc — the host driver of locus genotyping, included by mtr_abi.hip below motif_host.hip.inc (loci_round and its buffers, search_motifs_check_size): the flank
// search, the genotype and the partial genotype, their catalogue forms, the prepared catalogue, in the order they depend on each other.  What the
// loci's text and lengths decide - the checks and their words, the arrays of lengths, the codes - is loci_args.h; here the launches, the buffers
// and the looks at the device.

#define LA_CHK(check) do { if (!(check)) return MTR_ERR_BAD_ARG; } while (0)      // a check of loci_args.h: its reason is in ctx->err
using HostClock = std::chrono::steady_clock;
static double ms_since(HostClock::time_point t) { return std::chrono::duration<double, std::milli>(HostClock::now() - t).count(); }

// ---- flank search (flank_search.hip.inc) --------------------------------------------------------------------------------------------
// As the known-motif search: only the lengths decide the work - one argsort per call, the slots' masks and at most two work lists go up (one per
// word width), nothing comes back but the status word.  No scratch at all.
// the eight masks (FL_MASKS) of a slot's pattern, as both flank kernels take them (the 32-bit masks are their low halves), and the word it runs in
static void flank_slot_masks(const std::vector<uint8_t> &p, uint64_t *out)
{
    const int m = (int)p.size();
    const FbvMasks<uint64_t> eq = fbv_masks<uint64_t>(p.data(), m, 0), rev = fbv_masks<uint64_t>(p.data(), m, 1);
    const uint64_t v[FL_MASKS] = { eq.a, eq.c, eq.g, eq.t, rev.a, rev.c, rev.g, rev.t };
    std::copy(v, v + FL_MASKS, out);
}
static bool flank_is_wide(const mtr_ctx *ctx, int m) { return !(m <= 32 && ctx->sw.flank_word != 64); }

// every slot's pattern against every read: ctx->d_fl_res[read * S + slot][FL_RES], complete when this returns
static mtr_status flank_scan(mtr_ctx *ctx, const std::vector<std::vector<uint8_t>> &pat)
{
    const int n = ctx->n_reads;
    const size_t S = pat.size(), nr = (size_t)n;
    std::vector<int32_t> order(nr);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return ctx->lens[(size_t)x] > ctx->lens[(size_t)y]; });
    // the work lists: groups of 64 reads of the order per slot, the slots by the word their pattern needs
    std::vector<uint64_t> masks(S * FL_MASKS); std::vector<int32_t> plen(S);
    std::vector<int32_t> l_slot[2]; std::vector<int64_t> l_first[2];
    const int64_t groups = ((int64_t)n + 63) / 64;
    for (int k = 0; k < 2; k++) l_first[k].push_back(0);
    for (size_t slot = 0; slot < S; slot++) {
        const int m = (int)pat[slot].size();
        flank_slot_masks(pat[slot], masks.data() + slot * FL_MASKS);
        plen[slot] = m;
        const int k = flank_is_wide(ctx, m) ? 1 : 0;
        l_slot[k].push_back((int32_t)slot); l_first[k].push_back(l_first[k].back() + groups);
    }
    // device copies: d_fl_i32 = order | plen | the lists' slots, d_fl_i64 = masks | the lists' firsts
    HIPCHK(ctx->d_fl_i32.ensure((nr + 3 * S) * 4)); HIPCHK(ctx->d_fl_i64.ensure((S * FL_MASKS + 2 * (S + 1)) * 8));
    HIPCHK(ctx->d_fl_res.ensure(nr * S * FL_RES * 4)); HIPCHK(ctx->d_fl_status.ensure(4)); HIPCHK(ctx->d_fl_counter.ensure(2 * 8));
    int32_t *d_order = ctx->d_fl_i32, *d_plen = d_order + nr, *d_slots = d_plen + S;
    int64_t *d_masks = ctx->d_fl_i64, *d_firsts = d_masks + S * FL_MASKS;
    HIPCHK(copy_sync(ctx, d_order, order.data(), nr * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_plen, plen.data(), S * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, d_masks, masks.data(), S * FL_MASKS * 8, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; k++) {
        if (l_slot[k].empty()) continue;
        HIPCHK(copy_sync(ctx, d_slots + (size_t)k * S, l_slot[k].data(), l_slot[k].size() * 4, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(ctx, d_firsts + (size_t)k * (S + 1), l_first[k].data(), l_first[k].size() * 8, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemsetAsync(ctx->d_fl_status, 0, 4, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_fl_counter, 0, 2 * 8, ctx->stream));
    FlankArgs a{};
    a.b.packed = ctx->d_packed; a.b.woff = ctx->d_woff; a.b.lens = ctx->d_lens; a.b.order = d_order; a.b.n_reads = n;
    a.order = d_order; a.n_reads = n; a.n_slots = (int32_t)S; a.masks = (const uint64_t *)d_masks; a.plen = d_plen; a.res = ctx->d_fl_res; a.status = ctx->d_fl_status;
    for (int k = 0; k < 2; k++) {
        if (l_slot[k].empty()) continue;
        a.work = { d_slots + (size_t)k * S, d_firsts + (size_t)k * (S + 1), (int32_t)l_slot[k].size(), l_first[k].back() };
        a.counter = (unsigned long long *)ctx->d_fl_counter + k;
        size_t total = 0;
        const int waves = pick_waves(ctx, (int)std::min<int64_t>(l_first[k].back(), INT32_MAX), 16, 0, &total);
        DBG("flank scan: %d-bit word: %zu slots, %lld groups, %d wavefronts", k ? 64 : 32, l_slot[k].size(), (long long)l_first[k].back(), waves);
        if (k == 0) hipLaunchKernelGGL(mtr_k_flank_lanes<uint32_t>, dim3((unsigned)waves), dim3(64), 0, ctx->stream, a);
        else hipLaunchKernelGGL(mtr_k_flank_lanes<uint64_t>, dim3((unsigned)waves), dim3(64), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
    }
    int32_t dev = 0;
    HIPCHK(copy_sync(ctx, &dev, ctx->d_fl_status, 4, hipMemcpyDeviceToHost));
    if (dev != DEV_OK) { ctx->err = "the flank search failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    return MTR_OK;
}

extern "C" mtr_status mtr_search_flanks_device(mtr_ctx *ctx, const char *patterns, const int64_t *pattern_off, int32_t n_patterns, int32_t both_strands,
                                               const mtr_flank_hits_dst *dst, int64_t *out_hits)
{
    if (!ctx || !out_hits) return MTR_ERR_BAD_ARG;
    *out_hits = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    if (n_patterns <= 0) { ctx->err = "n_patterns = " + std::to_string(n_patterns) + ": at least one pattern is needed"; return MTR_ERR_BAD_ARG; }
    if (!patterns || !pattern_off) { ctx->err = "patterns or pattern_off is NULL"; return MTR_ERR_BAD_ARG; }
    const int ns = both_strands ? 2 : 1;
    for (int32_t k = 0; k < n_patterns; k++)
        if (pattern_off[k + 1] < pattern_off[k]) { ctx->err = "pattern_off decreases at pattern " + std::to_string(k); return MTR_ERR_BAD_ARG; }
    std::vector<std::vector<uint8_t>> pat;
    for (int32_t k = 0; k < n_patterns; k++) {
        const char *s = patterns + pattern_off[k];
        const int64_t len = pattern_off[k + 1] - pattern_off[k], t = la_seq_check(true, s, len);
        if (t < len) { ctx->err = la_refusal("pattern " + std::to_string(k), true, t, s, len); return MTR_ERR_BAD_ARG; }
        const std::vector<uint8_t> codes = la_codes(s, len);
        pat.push_back(codes);
        if (ns == 2) pat.push_back(revcomp_codes(codes));
    }
    const int64_t H = (int64_t)ctx->n_reads * n_patterns;
    if (H > (int64_t)INT32_MAX) { ctx->err = std::to_string(ctx->n_reads) + " reads x " + std::to_string(n_patterns) + " patterns are more than 2^31 - 1 hits"; return MTR_ERR_BAD_ARG; }
    *out_hits = H;
    if (!dst) return MTR_OK;
    if (dst->cap_hits < H) { ctx->err = "destination holds " + std::to_string(dst->cap_hits) + " hits, " + std::to_string(H) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->dist || !dst->start || !dst->end || !dst->strand) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    { mtr_status st = flank_scan(ctx, pat); if (st != MTR_OK) return st; }
    const FlankHitsOut out = { dst->dist, dst->start, dst->end, dst->strand };
    hipLaunchKernelGGL(mtr_k_flank_pack, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t *)ctx->d_fl_res, (int32_t)ns, H, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- the loci's checks (loci_args.h) ---------------------------------------------------------------------------------------------------
// what a text-taking call holds of its loci once they are accepted: what their lengths decide, the motifs side by side as the search takes
// them (L.mot_off), the four flank patterns of every locus (A, B, rc A, rc B) as codes
struct LociText { LociLengths L; std::string mot; std::vector<std::vector<uint8_t>> pat; };

// The genotype's checks of its arguments (la_check_genotype, after the batch's); on MTR_OK the motifs' text and the flanks' codes beside L
static mtr_status genotype_check_args(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist, int32_t gain, int32_t mismatch,
                                      int32_t indel, LociText &lt)
{
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    LA_CHK(la_check_genotype(ctx->n_reads, seqs, seq_off, n_loci, max_flank_dist, gain, mismatch, indel, lt.L, ctx->err));
    lt.mot.clear();
    for (size_t l = 0; l < (size_t)n_loci; l++) lt.mot.append(seqs + seq_off[3 * l + 1], (size_t)lt.L.ulen[l]);
    la_flank_patterns(seqs, seq_off, n_loci, lt.pat);
    return MTR_OK;
}

// the partial genotype's checks after the genotype's: a motif over 32 bases (naming the locus), then max_tail
static mtr_status partial_check_args(mtr_ctx *ctx, const std::vector<int64_t> &mot_off, int32_t n_loci, int32_t max_tail)
{
    for (int32_t l = 0; l < n_loci; l++)
        if (mot_off[(size_t)l + 1] - mot_off[(size_t)l] > MDP_MAX_U) {
            ctx->err = "locus " + std::to_string(l) + ": a motif of " + std::to_string(mot_off[(size_t)l + 1] - mot_off[(size_t)l]) + " bases, the partial genotype takes at most " + std::to_string(MDP_MAX_U);
            return MTR_ERR_BAD_ARG;
        }
    if (max_tail < 0) { ctx->err = "max_tail = " + std::to_string(max_tail) + ": at least 0"; return MTR_ERR_BAD_ARG; }
    return MTR_OK;
}

// ---- the alignment step of the genotype and of the catalogue genotype ---------------------------------------------------------------------
// The N intervals in ctx->d_gt_iv (the longest of max_len bases, counted in ctx->gt.state) through one round of the locus search's path over
// 2 * n_loci single-strand motifs; their hits are in ctx->gt.res on MTR_OK.
// the 2 * n_loci single-strand motif slots on the device - the slots' codes, their offsets, their 2-bit forms - and the offsets on the host
// cat_id: the prepared catalogue they belong to (mtr_catalog::id), 0 for tables a text-taking call made for itself
struct GtTables { const uint8_t *d_units; const int32_t *d_uoff; const uint64_t *d_bits; const std::vector<int32_t> *unit_off; uint64_t cat_id; };

// The alignment step from the device tables, whoever made them: the lane slots of this call's MTR_TEST_MOTIF_LANE_MAX from the units' lengths
// (the context's gt.i32 behind the text-taking calls' unit_off: slot_q | q_slot - a prepared catalogue is never written to), the round, and
// one look at the device: the status.
static mtr_status genotype_align_tables(mtr_ctx *ctx, const GtTables &tb, int32_t n_loci, int64_t N, int max_len, int32_t gain, int32_t mismatch, int32_t indel, const char *who)
{
    const int M2 = 2 * n_loci, lane_max = ctx->sw.motif_lane_max;
    LociRoundBufs &gt = ctx->gt;
    const LociRoundLayout at = loci_slot_layout((size_t)M2);                                // nq is not known yet
    HIPCHK(gt.i32.ensure(at.i32_bytes));
    int32_t *d_slot_q = gt.i32 + at.slot_q;
    // the lane slots: a prepared catalogue's, once derived and uploaded for this lane_max, stay in the context (its gt.i32 at this address)
    // until another catalogue, another lane_max or a text-taking call (cat_id = 0) takes their place; batch after batch sends nothing
    if (!(tb.cat_id != 0 && ctx->gt_ls && ctx->gt_ls_cat == tb.cat_id && ctx->gt_ls_lane_max == lane_max && ctx->gt_ls_at == d_slot_q)) {
        ctx->gt_ls_cat = 0;
        const std::shared_ptr<const LaneSlots> fresh = std::make_shared<const LaneSlots>(lane_slots(*tb.unit_off, M2, lane_max));
        { mtr_status r = upload_lane_slots(ctx, *fresh, d_slot_q, gt.i32 + at.q_slot); if (r != MTR_OK) return r; }
        ctx->gt_ls = fresh; ctx->gt_ls_cat = tb.cat_id; ctx->gt_ls_lane_max = lane_max; ctx->gt_ls_at = d_slot_q;
    }
    const LaneSlots &ls = *ctx->gt_ls;
    LociArgs a{};
    { mtr_status r = loci_round_bufs(ctx, gt, (size_t)M2, ls.q_slot.size(), (size_t)N, a); if (r != MTR_OK) return r; }
    a.iv = ctx->d_gt_iv; a.n_iv = (int32_t)N;
    a.n_motifs = M2; a.n_strands = 1; a.G = gain; a.MM = mismatch; a.D = indel;
    a.units = tb.d_units; a.unit_off = tb.d_uoff; a.bits = tb.d_bits;
    { mtr_status r = loci_round(ctx, a, ls, N, max_len, (unsigned long long *)gt.counter, who, 0); if (r != MTR_OK) return r; }
    // the status before the columns: a failed genotype writes nothing
    int32_t st[LOCI_STATE];
    return loci_round_status(ctx, gt, st, "genotype", "genotype's alignments", "");
}

// The alignment step of a text-taking call: the slots - locus l as given (2 * l) and reverse-complemented (2 * l + 1), one strand each - made
// here and sent up (gt.i32's unit_off, gt.i64, gt.units; the two lists behind unit_off are genotype_align_tables')
static mtr_status genotype_align(mtr_ctx *ctx, const std::string &mot, const std::vector<int64_t> &mot_off, int32_t n_loci, int64_t N, int max_len,
                                 int32_t gain, int32_t mismatch, int32_t indel, const char *who)
{
    SlotTables t;
    motif_slots(mot.data(), mot_off.data(), n_loci, 2, t.units, t.unit_off, t.bits);
    LociRoundBufs &gt = ctx->gt;
    HIPCHK(gt.i32.ensure(loci_slot_layout(t.bits.size()).i32_bytes));
    { mtr_status r = upload_slot_tables(ctx, t, gt.i32, gt.i64, gt.units); if (r != MTR_OK) return r; }
    const GtTables tb = { gt.units, gt.i32, (const uint64_t *)(int64_t *)gt.i64, &t.unit_off, 0 };
    return genotype_align_tables(ctx, tb, n_loci, N, max_len, gain, mismatch, indel, who);
}

// ---- locus genotyping (genotype.hip.inc) --------------------------------------------------------------------------------------------
// The flank step over four slots per locus, the pairing, one look at the device (how many windows, their longest), one round of the locus
// search's kernels over 2 * n_loci single-strand motifs (sized as mtr_search_motif_loci_device sizes a round), the columns.
extern "C" mtr_status mtr_genotype_loci_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist,
                                               int32_t gain, int32_t mismatch, int32_t indel, const mtr_genotypes_dst *dst, int64_t *out_rows)
{
    if (!ctx || !out_rows) return MTR_ERR_BAD_ARG;
    *out_rows = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    LociText lt;
    { mtr_status st = genotype_check_args(ctx, seqs, seq_off, n_loci, max_flank_dist, gain, mismatch, indel, lt); if (st != MTR_OK) return st; }
    const int n = ctx->n_reads;
    const int64_t rows = (int64_t)n * n_loci;
    { mtr_status st = search_motifs_check_size(ctx, lt.L.mot_off.data(), n_loci); if (st != MTR_OK) return st; }
    *out_rows = rows;
    if (!dst) return MTR_OK;
    if (dst->cap_rows < rows) { ctx->err = "destination holds " + std::to_string(dst->cap_rows) + " rows, " + std::to_string(rows) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->spanning || !dst->orientation || !dst->flank_dist || !dst->window || !dst->fields || !dst->score || !dst->ratio) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    { mtr_status st = flank_scan(ctx, lt.pat); if (st != MTR_OK) return st; }
    // the pairing
    HIPCHK(ctx->gt.state.ensure(LOCI_STATE * 4)); HIPCHK(ctx->d_gt_pair.ensure((size_t)rows * GT_PAIR * 4)); HIPCHK(ctx->d_gt_iv.ensure((size_t)rows * sizeof(LociIv)));
    HIPCHK(hipMemsetAsync(ctx->gt.state, 0, LOCI_STATE * 4, ctx->stream));
    const dim3 per_row((unsigned)((rows + 255) / 256)), b256(256);
    const GenoPairArgs ga = { ctx->d_fl_res, n_loci, max_flank_dist, rows, ctx->d_gt_pair, ctx->d_gt_iv, (int32_t)rows, ctx->gt.state };
    hipLaunchKernelGGL(mtr_k_geno_pair, per_row, b256, 0, ctx->stream, ga);
    HIPCHK(hipGetLastError());
    int32_t st[LOCI_STATE];
    HIPCHK(copy_sync(ctx, st, ctx->gt.state, sizeof st, hipMemcpyDeviceToHost));
    const int64_t N = st[LOCI_NEXT];
    const int max_len = st[LOCI_MAXLEN];
    if (st[LOCI_STATUS] != DEV_OK || N < 0 || N > rows || max_len < 0 || max_len > ctx->Lmax || (N > 0) != (max_len > 0)) {
        ctx->err = "the genotype's pairing failed on the device (status " + std::to_string(st[LOCI_STATUS]) + ")"; return MTR_ERR_HIP;
    }
    if (N > 0) { mtr_status r = genotype_align(ctx, lt.mot, lt.L.mot_off, n_loci, N, max_len, gain, mismatch, indel, "genotype_loci"); if (r != MTR_OK) return r; }
    const GenotypesOut out = { dst->spanning, dst->orientation, dst->flank_dist, dst->window, dst->fields, dst->score, dst->ratio };
    hipLaunchKernelGGL(mtr_k_geno_out, per_row, b256, 0, ctx->stream, (const int32_t *)ctx->d_gt_pair, (const int32_t *)ctx->gt.res, rows, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- the catalogue calls: the index, the front, the kept rows, the tail -----------------------------------------------------------------------
// The genotype's checks; the seed index built on the host (sorted entries, a table of the distinct codes, the filter bitmap) and sent up, or a
// prepared catalogue's; the front, common to both kinds (catalog_front): the scan in two passes around one look at the device (the hits), the
// candidates counted and a second look (the candidates); the kind's middle (genotype_catalog_rows, partial_catalog_rows), which leaves its rows
// in the context's columns; the tail (catalog_finish): the stream's end and the statistics.  Every buffer is sized by the reads, by the loci, or
// by what the scan found: none by reads x loci.
// The seed index of a catalogue call, as it lies in ctx->d_ct_ix (filter | key | run | entries | the slots' lengths), and what the host knows of it
struct CatIndex {
    size_t E = 0, distinct = 0, fwords = 0; uint32_t cap = 0; int fbits = 0;
    bool narrow = false, wide = false;                       // a slot of either flank word exists
    const uint32_t *d_filter = nullptr, *d_key = nullptr; const int32_t *d_run = nullptr, *d_ent = nullptr, *d_plen = nullptr;
    const uint64_t *d_masks = nullptr;                       // the slots' masks: ctx->d_ct_masks, or a prepared catalogue's
};

// A prepared catalogue (mtr_catalog_create): what depends on the loci alone.  On the host what lengths decide; on the device, in buffers of its
// own (no context owns them: any context of the device may read them, none writes), the index as CatIndex points into it, the slots' masks,
// the genotype's 2 * n_loci single-strand motif slots (GtTables) and the partial genotype's variants (vbits, ulen).
struct mtr_catalog {
    uint64_t id = 0;                                        // never 0 and never given twice in a process: what a context remembers a catalogue by
    int device = 0; int32_t n_loci = 0, max_flank_dist = 0, seed_len = 0;
    size_t E = 0, distinct = 0, fwords = 0; uint32_t cap = 0; int fbits = 0;
    int64_t n_short = 0, n_long = 0;                        // slots of at most / of more than 32 bases: which flank words a call launches
    int64_t first_long_motif = -1;
    std::vector<int64_t> mot_off;                           // [n_loci + 1]: the motifs' lengths as search_motifs_check_size takes them
    std::vector<int32_t> unit_off;                          // [2 * n_loci + 1]: the motif slots' offsets (lane_slots)
    DevBuf<uint32_t> d_filter, d_key; DevBuf<int32_t> d_run, d_ent, d_plen, d_uoff, d_ulen; DevBuf<uint64_t> d_masks, d_ubits, d_vbits; DevBuf<uint8_t> d_units;
    size_t device_bytes() const { return d_filter.cap + d_key.cap + d_run.cap + d_ent.cap + d_plen.cap + d_uoff.cap + d_ulen.cap + d_masks.cap + d_ubits.cap + d_vbits.cap + d_units.cap; }
};
static GtTables catalog_gt_tables(const mtr_catalog *cat) { return { cat->d_units, cat->d_uoff, cat->d_ubits, &cat->unit_off, cat->id }; }

// what a catalogue call runs on beside the index: the motifs as text (the text-taking calls), or a prepared catalogue's tables
struct CatMotifs { const std::string *mot; const std::vector<int64_t> *mot_off; const mtr_catalog *cat; };

// What every catalogue call needs beside an index, whichever made it: the reads' count and offset buffers sized, the status and the filter's
// count zeroed
static mtr_status catalog_scan_buffers(mtr_ctx *ctx)
{
    const size_t nr = (size_t)ctx->n_reads;
    HIPCHK(ctx->d_ct_count.ensure(2 * nr * 4)); HIPCHK(ctx->d_ct_off.ensure(2 * (nr + 1) * 8)); HIPCHK(ctx->d_ct_status.ensure(4)); HIPCHK(ctx->d_ct_passed.ensure(8));
    HIPCHK(hipMemsetAsync(ctx->d_ct_status, 0, 4, ctx->stream)); HIPCHK(hipMemsetAsync(ctx->d_ct_passed, 0, 8, ctx->stream));
    return MTR_OK;
}

// The index built on the host and sent up: the entries (code, locus * 4 + slot) sorted and made distinct, a table slot per distinct code, the
// filter over the codes (sized as the device build sizes them: cb_table_cap, cb_filter_bits), the slots' masks (ctx->d_ct_masks) and lengths;
// the reads' count and offset buffers sized, the status and the filter's count zeroed.  The copies are synchronous.
static_assert(CAT_FILTER_MIN_BITS == CB_FILTER_MIN_BITS && CAT_FILTER_MAX_BITS == CB_FILTER_MAX_BITS, "the scan's filter and the builds' agree on its sizes");
static mtr_status catalog_index(mtr_ctx *ctx, const std::vector<std::vector<uint8_t>> &pat, int seeds, int q, CatIndex &o)
{
    const size_t S = pat.size();
    std::vector<std::pair<uint32_t, int32_t>> ent;
    ent.reserve(S * (size_t)seeds);
    std::vector<uint64_t> masks(S * FL_MASKS); std::vector<int32_t> plen(S);
    for (size_t slot = 0; slot < S; slot++) {
        const int m = (int)pat[slot].size();
        for (int i = 0; i < seeds; i++) ent.push_back({ si_seed_code(pat[slot].data() + si_seed_offset(i, q), q), (int32_t)slot });
        flank_slot_masks(pat[slot], masks.data() + slot * FL_MASKS);
        plen[slot] = m;
        (flank_is_wide(ctx, m) ? o.wide : o.narrow) = true;
    }
    std::sort(ent.begin(), ent.end());
    ent.erase(std::unique(ent.begin(), ent.end()), ent.end());
    const size_t E = ent.size();
    size_t distinct = 0;
    for (size_t e = 0; e < E; e++) distinct += e == 0 || ent[e].first != ent[e - 1].first;
    const uint32_t cap = cb_table_cap(distinct);
    const int fbits = cb_filter_bits(distinct);
    const size_t fwords = ((size_t)1 << fbits) / 32;
    std::vector<uint32_t> ix(fwords + 3 * (size_t)cap + E + S, 0);                                     // filter | key | run | entries | plen
    uint32_t *h_filter = ix.data(), *h_key = h_filter + fwords; int32_t *h_run = (int32_t *)(h_key + cap), *h_ent = h_run + 2 * (size_t)cap, *h_plen = h_ent + E;
    for (size_t e = 0, first = 0; e < E; e++) {
        h_ent[e] = ent[e].second;
        if (e + 1 < E && ent[e + 1].first == ent[e].first) continue;
        si_filter_set(h_filter, fbits, ent[e].first);
        if (!si_insert(h_key, h_run, cap, ent[e].first, (int32_t)first, (int32_t)(e + 1 - first))) { ctx->err = "the seed table is full"; return MTR_ERR_HIP; }
        first = e + 1;
    }
    std::copy(plen.begin(), plen.end(), h_plen);
    HIPCHK(ctx->d_ct_ix.ensure(ix.size() * 4)); HIPCHK(ctx->d_ct_masks.ensure(masks.size() * 8));
    HIPCHK(copy_sync(ctx, ctx->d_ct_ix, ix.data(), ix.size() * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, ctx->d_ct_masks, masks.data(), masks.size() * 8, hipMemcpyHostToDevice));
    { mtr_status st = catalog_scan_buffers(ctx); if (st != MTR_OK) return st; }
    o.d_masks = ctx->d_ct_masks;
    o.E = E; o.distinct = distinct; o.fwords = fwords; o.cap = cap; o.fbits = fbits;
    o.d_filter = (const uint32_t *)(int32_t *)ctx->d_ct_ix; o.d_key = o.d_filter + fwords;
    o.d_run = (const int32_t *)(o.d_key + cap); o.d_ent = o.d_run + 2 * (size_t)cap; o.d_plen = o.d_ent + E;
    return MTR_OK;
}

// what the front leaves to a middle and to the tail; sa.b: the reads, for the flank kernels; t_rest: the mark the rest of the call is timed from
struct CatFront { CatScanArgs sa{}; int64_t H = 0, Cn = 0; unsigned long long passed = 0; double ms_scan = 0; HostClock::time_point t_rest; };

// The front of both kinds: the scan's count pass and a look at the device (the hits, then the filter's count); for H > 0 the scan's fill pass, the
// kind's candidates kernel counting (`cands` over `ca`, whose common fields are set here: the middle fills with the same block), their offsets,
// and a second look (the candidates).  who: the call, for MTR_DEBUG; whose: "the catalogue's" or "the partial catalogue's", for the reasons.
template <typename CandArgs>
static mtr_status catalog_front(mtr_ctx *ctx, const CatIndex &ix, int q, const char *who, const char *whose, void (*cands)(CandArgs), CandArgs &ca, CatFront &f)
{
    const int n = ctx->n_reads;
    const size_t nr = (size_t)n;
    int32_t *hit_count = ctx->d_ct_count, *cand_count = hit_count + nr;
    int64_t *hit_off = ctx->d_ct_off, *cand_off = hit_off + nr + 1;
    const dim3 per_read((unsigned)n), b64(64), one(1), b1024(1024);
    const auto t_scan = HostClock::now();
    CatScanArgs &sa = f.sa;
    sa.b.packed = ctx->d_packed; sa.b.woff = ctx->d_woff; sa.b.lens = ctx->d_lens; sa.b.order = nullptr; sa.b.n_reads = n;
    sa.ix = { ix.d_filter, ix.fbits, ix.d_key, ix.d_run, ix.cap }; sa.ent = ix.d_ent; sa.q = q; sa.fill = 0;
    sa.hit_count = hit_count; sa.hit_off = hit_off; sa.hits = nullptr; sa.passed = ctx->d_ct_passed;
    hipLaunchKernelGGL(mtr_k_cat_scan, per_read, b64, 0, ctx->stream, sa);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)hit_count, (int64_t)n, hit_off);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, &f.H, hit_off + nr, 8, hipMemcpyDeviceToHost));
    if (f.H < 0 || f.H >= (int64_t)INT32_MAX) { ctx->err = "2^31 - 1 seed hits or more (a read's count saturates there)"; return MTR_ERR_OVERFLOW; }
    f.ms_scan = ms_since(t_scan);                                    // the first scan pass and the offsets, up to the look that ends them
    f.t_rest = HostClock::now();
    HIPCHK(copy_sync(ctx, &f.passed, ctx->d_ct_passed, 8, hipMemcpyDeviceToHost));
    DBG("%s: %zu entries of %zu codes, table of %u slots, filter of 2^%d bits; the filter passed %llu positions, %lld hits", who, ix.E, ix.distinct, ix.cap, ix.fbits, f.passed, (long long)f.H);
    if (f.H == 0) return MTR_OK;
    HIPCHK(ctx->d_ct_hits.ensure((size_t)f.H * 4)); HIPCHK(ctx->d_ct_head.ensure((size_t)f.H));
    sa.fill = 1; sa.hits = ctx->d_ct_hits;
    hipLaunchKernelGGL(mtr_k_cat_scan, per_read, b64, 0, ctx->stream, sa);
    ca.n_reads = n; ca.fill = 0; ca.hit_off = hit_off; ca.hits = ctx->d_ct_hits; ca.head = ctx->d_ct_head; ca.cand_count = cand_count; ca.cand_off = cand_off;
    hipLaunchKernelGGL(cands, per_read, b64, 0, ctx->stream, ca);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)cand_count, (int64_t)n, cand_off);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, &f.Cn, cand_off + nr, 8, hipMemcpyDeviceToHost));
    if (f.Cn < 0 || f.Cn > f.H) { ctx->err = std::string(whose) + " candidate lists are inconsistent"; return MTR_ERR_HIP; }
    if (f.Cn > (int64_t)INT32_MAX / 2) { ctx->err = std::to_string(f.Cn) + " candidates are more than 2^30 - 1"; return MTR_ERR_OVERFLOW; }
    return MTR_OK;
}

// The tail of both kinds: the stream's end, R rows kept, the statistics of mtr_test_catalog_stats / mtr_test_partial_catalog_stats
static mtr_status catalog_finish(mtr_ctx *ctx, CatKept &kept, const CatFront &f, int q, double ms_index, int64_t R, int64_t *out_rows, int64_t *out_candidates)
{
    HIPCHK(hipStreamSynchronize(ctx->stream));
    kept.ready = true; kept.rows = R;
    int64_t positions = 0;
    for (int i = 0; i < ctx->n_reads; i++) positions += std::max(0, ctx->lens[(size_t)i] - q + 1);
    kept.counts[0] = positions; kept.counts[1] = (int64_t)f.passed; kept.counts[2] = f.H; kept.counts[3] = f.Cn;
    kept.ms[0] = ms_index; kept.ms[1] = f.ms_scan; kept.ms[2] = ms_since(f.t_rest);
    *out_rows = R; *out_candidates = f.Cn;
    return MTR_OK;
}

// The kept rows of either kind: CAT_ROW_COLS columns of the context, named by the kind's enum, row_bytes[c] bytes a row; the call that makes them and their copy walk that table
enum { GC_READ, GC_LOCUS, GC_SPANNING, GC_ORIENTATION, GC_FDIST, GC_WINDOW, GC_FIELDS, GC_SCORE, GC_RATIO };
static const size_t gc_row_bytes[CAT_ROW_COLS] = { 4, 4, 1, 1, 8, 8, 32, 4, 4 };
enum { PK_READ, PK_LOCUS, PK_PARTIAL, PK_SLOT, PK_FDIST, PK_WINDOW, PK_EXT, PK_RATIO, PK_OPEN };
static const size_t pk_row_bytes[CAT_ROW_COLS] = { 4, 4, 1, 1, 4, 8, 24, 4, 1 };
template <typename T> static T *kept_col(DevBuf<uint8_t> *cols, int c) { return (T *)(uint8_t *)cols[c]; }

// a *_copy_device from its destination's columns on (dst[c] takes cols[c])
static mtr_status kept_rows_copy(mtr_ctx *ctx, const CatKept &kept, const DevBuf<uint8_t> *cols, const size_t *row_bytes, void *const *dst, int64_t cap_rows)
{
    const int64_t R = kept.rows;
    if (cap_rows < R) { ctx->err = "destination holds " + std::to_string(cap_rows) + " rows, " + std::to_string(R) + " needed"; return MTR_ERR_OVERFLOW; }
    if (R == 0) return MTR_OK;
    for (int c = 0; c < CAT_ROW_COLS; c++)
        if (!dst[c]) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    for (int c = 0; c < CAT_ROW_COLS; c++) HIPCHK(hipMemcpyAsync(dst[c], cols[c], (size_t)R * row_bytes[c], hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- catalogue genotype (catalog.hip.inc) -------------------------------------------------------------------------------------------
// The middle of the catalogue genotype, for Cn > 0 candidates: their fill pass, their two flank scans each, the pairing, a third look (the
// windows, their longest, the rows), the genotype's alignment step, the R rows into the context's columns.
static mtr_status genotype_catalog_rows(mtr_ctx *ctx, const CatIndex &ix, const CatMotifs &cm, const CatFront &f, CatCandArgs &ca, int32_t n_loci, int32_t max_flank_dist,
                                        int32_t gain, int32_t mismatch, int32_t indel, int64_t *out_R)
{
    const int64_t Cn = f.Cn;
    const size_t nc = (size_t)Cn;
    const dim3 per_read((unsigned)ctx->n_reads), b64(64), b256(256), one(1), b1024(1024);
    HIPCHK(ctx->d_ct_cand.ensure(3 * nc * 4)); HIPCHK(ctx->d_ct_flank.ensure(2 * nc * FL_RES * 4)); HIPCHK(ctx->d_ct_rowoff.ensure((nc + 1) * 8));
    int32_t *cand_read = ctx->d_ct_cand, *cand_key = cand_read + nc, *span = cand_key + nc;
    int64_t *row_off = ctx->d_ct_rowoff;
    ca.fill = 1; ca.cand_read = cand_read; ca.cand_key = cand_key;
    hipLaunchKernelGGL(mtr_k_cat_cands, per_read, b64, 0, ctx->stream, ca);
    // the candidates' two flank scans each
    CatFlankArgs fa{};
    fa.b = f.sa.b; fa.cand_read = cand_read; fa.cand_key = cand_key; fa.n_tasks = (int32_t)(2 * Cn);
    fa.masks = ix.d_masks; fa.plen = ix.d_plen; fa.all_wide = ctx->sw.flank_word == 64; fa.res = ctx->d_ct_flank; fa.status = ctx->d_ct_status;
    const dim3 per_task((unsigned)((2 * nc + 63) / 64));
    if (ix.narrow) hipLaunchKernelGGL(mtr_k_cat_flank<uint32_t>, per_task, b64, 0, ctx->stream, fa);
    if (ix.wide) hipLaunchKernelGGL(mtr_k_cat_flank<uint64_t>, per_task, b64, 0, ctx->stream, fa);
    // the pairing, and the rows' places
    HIPCHK(ctx->gt.state.ensure(LOCI_STATE * 4)); HIPCHK(ctx->d_gt_pair.ensure(nc * GT_PAIR * 4)); HIPCHK(ctx->d_gt_iv.ensure(nc * sizeof(LociIv)));
    HIPCHK(hipMemsetAsync(ctx->gt.state, 0, LOCI_STATE * 4, ctx->stream));
    const dim3 per_cand((unsigned)((nc + 255) / 256));
    const CatPairArgs pa = { cand_read, cand_key, (int32_t)Cn, ctx->d_ct_flank, n_loci, max_flank_dist, ctx->d_gt_pair, span, ctx->d_gt_iv, (int32_t)Cn, ctx->gt.state };
    hipLaunchKernelGGL(mtr_k_cat_pair, per_cand, b256, 0, ctx->stream, pa);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)span, Cn, row_off);
    HIPCHK(hipGetLastError());
    int32_t st[LOCI_STATE], dev = 0;
    int64_t R = 0;
    HIPCHK(copy_sync(ctx, st, ctx->gt.state, sizeof st, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, &dev, ctx->d_ct_status, 4, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, &R, row_off + nc, 8, hipMemcpyDeviceToHost));
    const int64_t N = st[LOCI_NEXT];
    const int max_len = st[LOCI_MAXLEN];
    if (dev != DEV_OK) { ctx->err = "the catalogue's flank scans failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    if (st[LOCI_STATUS] != DEV_OK || R < 0 || R > Cn || N < 0 || N > R || max_len < 0 || max_len > ctx->Lmax || (N > 0) != (max_len > 0)) {
        ctx->err = "the catalogue's pairing failed on the device (status " + std::to_string(st[LOCI_STATUS]) + ")"; return MTR_ERR_HIP;
    }
    if (N > 0) {
        const mtr_status r = cm.cat ? genotype_align_tables(ctx, catalog_gt_tables(cm.cat), n_loci, N, max_len, gain, mismatch, indel, "genotype_catalog")
                                    : genotype_align(ctx, *cm.mot, *cm.mot_off, n_loci, N, max_len, gain, mismatch, indel, "genotype_catalog");
        if (r != MTR_OK) return r;
    }
    if (R > 0) {
        DevBuf<uint8_t> *k = ctx->d_gc;
        for (int c = 0; c < CAT_ROW_COLS; c++) HIPCHK(k[c].ensure((size_t)R * gc_row_bytes[c]));
        const CatRowsOut out = { kept_col<int32_t>(k, GC_READ), kept_col<int32_t>(k, GC_LOCUS),
                                 { kept_col<uint8_t>(k, GC_SPANNING), kept_col<uint8_t>(k, GC_ORIENTATION), kept_col<int32_t>(k, GC_FDIST), kept_col<int32_t>(k, GC_WINDOW),
                                   kept_col<int32_t>(k, GC_FIELDS), kept_col<int32_t>(k, GC_SCORE), kept_col<float>(k, GC_RATIO) } };
        hipLaunchKernelGGL(mtr_k_cat_out, per_cand, b256, 0, ctx->stream, (const int32_t *)cand_read, (const int32_t *)cand_key, (const int32_t *)ctx->d_gt_pair,
                           (const int32_t *)span, (const int64_t *)row_off, (const int32_t *)ctx->gt.res, (int32_t)Cn, out);
        HIPCHK(hipGetLastError());
    }
    *out_R = R;
    return MTR_OK;
}

extern "C" mtr_status mtr_test_catalog_stats(mtr_ctx *ctx, int64_t *counts, double *ms)
{
    if (!ctx || !counts || !ms) return MTR_ERR_BAD_ARG;
    if (!ctx->gc.ready) { ctx->err = "no catalogue call to report on"; return MTR_ERR_BAD_ARG; }
    std::copy(ctx->gc.counts, ctx->gc.counts + 4, counts); std::copy(ctx->gc.ms, ctx->gc.ms + 3, ms);
    return MTR_OK;
}

extern "C" mtr_status mtr_genotype_catalog_copy_device(mtr_ctx *ctx, const mtr_catalog_dst *dst)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (!ctx->gc.ready) { ctx->err = "no rows kept: mtr_genotype_catalog_device comes first (an upload discards what it kept)"; return MTR_ERR_BAD_ARG; }
    if (!dst) { ctx->err = "dst is NULL"; return MTR_ERR_BAD_ARG; }
    const mtr_genotypes_dst &g = dst->rows;
    void *const cols[CAT_ROW_COLS] = { dst->read, dst->locus, g.spanning, g.orientation, g.flank_dist, g.window, g.fields, g.score, g.ratio };      // the order of GC_*
    return kept_rows_copy(ctx, ctx->gc, ctx->d_gc, gc_row_bytes, cols, g.cap_rows);
}

// ---- partial genotype (partial.hip.inc) ------------------------------------------------------------------------------------------------
// The genotype's checks and its flank step, the pairing and the choice of slot, one look at the device (the status and every variant's number
// of tasks), one launch of the extension per bucket that has tasks, the columns.
extern "C" mtr_status mtr_genotype_partial_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist,
                                                  int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail, const mtr_partial_dst *dst, int64_t *out_rows)
{
    if (!ctx || !out_rows) return MTR_ERR_BAD_ARG;
    *out_rows = 0;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    LociText lt;
    { mtr_status st = genotype_check_args(ctx, seqs, seq_off, n_loci, max_flank_dist, gain, mismatch, indel, lt); if (st != MTR_OK) return st; }
    { mtr_status st = partial_check_args(ctx, lt.L.mot_off, n_loci, max_tail); if (st != MTR_OK) return st; }
    const int n = ctx->n_reads;
    const int64_t rows = (int64_t)n * n_loci;
    *out_rows = rows;
    if (!dst) return MTR_OK;
    if (dst->cap_rows < rows) { ctx->err = "destination holds " + std::to_string(dst->cap_rows) + " rows, " + std::to_string(rows) + " needed"; return MTR_ERR_OVERFLOW; }
    if (!dst->partial || !dst->slot || !dst->flank_dist || !dst->window || !dst->ext || !dst->ratio || !dst->open) { ctx->err = "a destination column is NULL"; return MTR_ERR_BAD_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    { mtr_status st = flank_scan(ctx, lt.pat); if (st != MTR_OK) return st; }
    // the variants of every locus: M, reversed M, rc M, reversed rc M, as motif_ext takes them
    const size_t V = (size_t)n_loci * 4, nl = (size_t)n_loci, nr = (size_t)n;
    std::vector<uint64_t> bits; std::vector<int32_t> ulen;
    partial_variants(lt.mot, lt.L.mot_off, n_loci, bits, ulen);
    // device copies: d_pt_i32 = status | count | ulen | the work lists' variants, d_pt_i64 = bits | the work lists' firsts (a list per bucket)
    HIPCHK(ctx->d_pt_i32.ensure((1 + 2 * V + nl) * 4)); HIPCHK(ctx->d_pt_i64.ensure((2 * V + 4) * 8));
    HIPCHK(ctx->d_pt_row.ensure((size_t)rows * PT_ROW * 4)); HIPCHK(ctx->d_pt_ext.ensure((size_t)rows * PT_EXT * 4)); HIPCHK(ctx->d_pt_task.ensure(V * nr * sizeof(PtTask)));
    int32_t *d_status = ctx->d_pt_i32, *d_count = d_status + 1, *d_ulen = d_count + V, *d_wslot = d_ulen + nl;
    int64_t *d_bits = ctx->d_pt_i64, *d_wfirst = d_bits + V;
    HIPCHK(hipMemsetAsync(d_status, 0, (1 + V) * 4, ctx->stream));
    HIPCHK(copy_sync(ctx, d_ulen, ulen.data(), nl * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_bits, bits.data(), V * 8, hipMemcpyHostToDevice));
    const dim3 per_row((unsigned)((rows + 255) / 256)), b256(256);
    const PartialPairArgs pa = { ctx->d_fl_res, ctx->d_lens, n_loci, max_flank_dist, n, rows, ctx->d_pt_row, ctx->d_pt_task, d_count, d_status };
    hipLaunchKernelGGL(mtr_k_partial_pair, per_row, b256, 0, ctx->stream, pa);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> head(1 + V);
    HIPCHK(copy_sync(ctx, head.data(), d_status, (1 + V) * 4, hipMemcpyDeviceToHost));
    bool sane = head[0] == DEV_OK;
    for (size_t v = 0; v < V; v++) sane = sane && head[1 + v] >= 0 && head[1 + v] <= n;
    if (!sane) { ctx->err = "the partial genotype's pairing failed on the device (status " + std::to_string(head[0]) + ")"; return MTR_ERR_HIP; }
    // a work list per bucket: entries (variant, first group) of the variants that have tasks
    std::vector<int32_t> wslot; std::vector<int64_t> wfirst;
    struct Launch { int ub; size_t slot_at, first_at; int32_t entries; int64_t groups; } launches[4];
    int n_launch = 0;
    for (int ub = 4; ub <= MDP_MAX_U; ub *= 2) {
        Launch la = { ub, wslot.size(), wfirst.size(), 0, 0 };
        for (size_t v = 0; v < V; v++)
            if (head[1 + v] > 0 && mdp_bucket(ulen[v >> 2]) == ub) { wslot.push_back((int32_t)v); wfirst.push_back(la.groups); la.entries++; la.groups += ((int64_t)head[1 + v] + 63) / 64; }
        wfirst.push_back(la.groups);
        if (la.entries > 0) launches[n_launch++] = la;
    }
    if (n_launch > 0) {
        HIPCHK(copy_sync(ctx, d_wslot, wslot.data(), wslot.size() * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, d_wfirst, wfirst.data(), wfirst.size() * 8, hipMemcpyHostToDevice));
        PartialExtArgs a{};
        a.b.packed = ctx->d_packed; a.b.woff = ctx->d_woff; a.b.lens = ctx->d_lens; a.b.order = nullptr; a.b.n_reads = n;
        a.tasks = ctx->d_pt_task; a.count = d_count; a.bits = (const uint64_t *)d_bits; a.ulen = d_ulen;
        a.n_reads = n; a.n_loci = n_loci; a.G = gain; a.MM = mismatch; a.D = indel; a.ext = ctx->d_pt_ext; a.status = d_status;
        for (int k = 0; k < n_launch; k++) {
            const Launch &la = launches[k];
            a.work = { d_wslot + la.slot_at, d_wfirst + la.first_at, la.entries, la.groups };
            DBG("partial genotype: bucket %d: %d variants, %lld groups", la.ub, la.entries, (long long)la.groups);
            LAUNCH_BY_BUCKET(mtr_k_ext_lanes, la.ub, dim3((unsigned)la.groups), dim3(64), ctx->stream, a);
            HIPCHK(hipGetLastError());
        }
        // the status before the columns: a failed call writes nothing
        int32_t dev = 0;
        HIPCHK(copy_sync(ctx, &dev, d_status, 4, hipMemcpyDeviceToHost));
        if (dev != DEV_OK) { ctx->err = "the partial genotype's extensions failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    }
    const PartialOut out = { dst->partial, dst->slot, dst->flank_dist, dst->window, dst->ext, dst->ratio, dst->open };
    hipLaunchKernelGGL(mtr_k_partial_out, per_row, b256, 0, ctx->stream, (const int32_t *)ctx->d_pt_row, (const int32_t *)ctx->d_pt_ext, (const int32_t *)d_ulen, n_loci, max_tail, rows, out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MTR_OK;
}

// ---- partial genotype at catalogue scale (partial_catalog.hip.inc) -----------------------------------------------------------------------
// The middle of the partial genotype at catalogue scale, for Cn > 0 candidates: their fill pass and their seeded slots as flank tasks (a third
// look: the tasks), the scans, the variants, the pairing, a fourth look (the status, the buckets' tasks, the rows); one launch of the extension per
// bucket that has tasks and the status again; the R rows into the context's columns.
static mtr_status partial_catalog_rows(mtr_ctx *ctx, const CatIndex &ix, const CatMotifs &cm, const CatFront &f, PtcCandArgs &ca, int32_t n_loci, int32_t max_flank_dist,
                                       int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail, int64_t *out_R)
{
    const int64_t Cn = f.Cn, H = f.H;
    const size_t nc = (size_t)Cn, nl = (size_t)n_loci;
    const dim3 per_read((unsigned)ctx->n_reads), b64(64), b256(256), one(1), b1024(1024);
    // the candidates, their seeded slots as flank tasks
    HIPCHK(ctx->d_pc_cand.ensure(5 * nc * 4)); HIPCHK(ctx->d_pc_toff.ensure((nc + 1) * 8)); HIPCHK(ctx->d_ct_flank.ensure(PT_SLOTS * nc * FL_RES * 4));
    HIPCHK(ctx->d_ct_rowoff.ensure((nc + 1) * 8));
    int32_t *cand_read = ctx->d_pc_cand, *cand_locus = cand_read + nc, *cand_mask = cand_locus + nc, *cand_slots = cand_mask + nc, *is_row = cand_slots + nc;
    int64_t *task_off = ctx->d_pc_toff, *row_off = ctx->d_ct_rowoff;
    ca.fill = 1; ca.cand_read = cand_read; ca.cand_locus = cand_locus; ca.cand_mask = cand_mask; ca.cand_slots = cand_slots;
    hipLaunchKernelGGL(mtr_k_ptc_cands, per_read, b64, 0, ctx->stream, ca);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)cand_slots, Cn, task_off);
    HIPCHK(hipGetLastError());
    int64_t F = 0;
    HIPCHK(copy_sync(ctx, &F, task_off + nc, 8, hipMemcpyDeviceToHost));
    if (F < Cn || F > PT_SLOTS * Cn || F > H) { ctx->err = "the partial catalogue's flank tasks are inconsistent"; return MTR_ERR_HIP; }
    HIPCHK(ctx->d_pc_ftask.ensure((size_t)F * 4));
    const dim3 per_cand((unsigned)((nc + 255) / 256));
    const PtcTaskArgs ta = { cand_mask, task_off, (int32_t)Cn, ctx->d_pc_ftask, ctx->d_ct_flank };
    hipLaunchKernelGGL(mtr_k_ptc_tasks, per_cand, b256, 0, ctx->stream, ta);
    PtcFlankArgs fa{};
    fa.b = f.sa.b; fa.cand_read = cand_read; fa.cand_locus = cand_locus; fa.n_cand = (int32_t)Cn; fa.tasks = ctx->d_pc_ftask; fa.n_tasks = (int32_t)F;
    fa.masks = ix.d_masks; fa.plen = ix.d_plen; fa.all_wide = ctx->sw.flank_word == 64; fa.res = ctx->d_ct_flank; fa.status = ctx->d_ct_status;
    const dim3 per_task((unsigned)(((size_t)F + 63) / 64));
    if (ix.narrow) hipLaunchKernelGGL(mtr_k_ptc_flank<uint32_t>, per_task, b64, 0, ctx->stream, fa);
    if (ix.wide) hipLaunchKernelGGL(mtr_k_ptc_flank<uint64_t>, per_task, b64, 0, ctx->stream, fa);
    // the variants; d_pc_i32 = status | count[4] | ulen, d_pc_i64 = bits
    // (a prepared catalogue brings its own bits and ulen; the text-taking call makes them here and keeps them behind its status words)
    HIPCHK(ctx->d_pc_i32.ensure((1 + PTC_BUCKETS + nl) * 4));
    HIPCHK(ctx->d_pc_row.ensure(nc * PT_ROW * 4)); HIPCHK(ctx->d_pc_ext.ensure(nc * PT_EXT * 4)); HIPCHK(ctx->d_pc_task.ensure(PTC_BUCKETS * nc * sizeof(PtTask)));
    int32_t *d_status = ctx->d_pc_i32, *d_count = d_status + 1;
    const int32_t *d_ulen = d_count + PTC_BUCKETS; const uint64_t *d_vbits = nullptr;
    HIPCHK(hipMemsetAsync(d_status, 0, (1 + PTC_BUCKETS) * 4, ctx->stream));
    if (cm.cat) { d_ulen = cm.cat->d_ulen; d_vbits = cm.cat->d_vbits; }
    else {
        std::vector<uint64_t> bits; std::vector<int32_t> ulen;
        partial_variants(*cm.mot, *cm.mot_off, n_loci, bits, ulen);
        HIPCHK(ctx->d_pc_i64.ensure(bits.size() * 8));
        HIPCHK(copy_sync(ctx, d_count + PTC_BUCKETS, ulen.data(), nl * 4, hipMemcpyHostToDevice)); HIPCHK(copy_sync(ctx, ctx->d_pc_i64, bits.data(), bits.size() * 8, hipMemcpyHostToDevice));
        d_vbits = (const uint64_t *)(int64_t *)ctx->d_pc_i64;
    }
    // the pairing, and the rows' places
    const PtcPairArgs pa = { cand_read, cand_locus, (int32_t)Cn, ctx->d_ct_flank, ctx->d_lens, d_ulen, max_flank_dist, ctx->d_pc_row, is_row, ctx->d_pc_task, d_count, d_status };
    hipLaunchKernelGGL(mtr_k_ptc_pair, per_cand, b256, 0, ctx->stream, pa);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)is_row, Cn, row_off);
    HIPCHK(hipGetLastError());
    int32_t head[1 + PTC_BUCKETS], dev = 0;
    int64_t R = 0;
    HIPCHK(copy_sync(ctx, head, d_status, sizeof head, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, &dev, ctx->d_ct_status, 4, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, &R, row_off + nc, 8, hipMemcpyDeviceToHost));
    if (dev != DEV_OK) { ctx->err = "the partial catalogue's flank scans failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    bool sane = head[0] == DEV_OK && R >= 0 && R <= Cn;
    int64_t tasks = 0;
    for (int b = 0; b < PTC_BUCKETS; b++) { sane = sane && head[1 + b] >= 0 && head[1 + b] <= Cn; tasks += head[1 + b]; }
    if (!sane || tasks > R) { ctx->err = "the partial catalogue's pairing failed on the device (status " + std::to_string(head[0]) + ")"; return MTR_ERR_HIP; }
    if (tasks > 0) {
        PtcExtArgs a{};
        a.b = f.sa.b; a.cand_read = cand_read; a.tasks = ctx->d_pc_task; a.count = d_count; a.n_cand = (int32_t)Cn;
        a.bits = d_vbits; a.ulen = d_ulen; a.G = gain; a.MM = mismatch; a.D = indel; a.ext = ctx->d_pc_ext; a.status = d_status;
        for (int b = 0; b < PTC_BUCKETS; b++) {
            if (head[1 + b] == 0) continue;
            DBG("genotype_partial_catalog: bucket %d: %d tasks", 4 << b, head[1 + b]);
            LAUNCH_BY_BUCKET(mtr_k_ptc_ext, 4 << b, dim3((unsigned)((head[1 + b] + 63) / 64)), b64, ctx->stream, a);
            HIPCHK(hipGetLastError());
        }
        // the status before anything is kept
        HIPCHK(copy_sync(ctx, &dev, d_status, 4, hipMemcpyDeviceToHost));
        if (dev != DEV_OK) { ctx->err = "the partial catalogue's extensions failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    }
    if (R > 0) {
        DevBuf<uint8_t> *k = ctx->d_pk;
        for (int c = 0; c < CAT_ROW_COLS; c++) HIPCHK(k[c].ensure((size_t)R * pk_row_bytes[c]));
        PtcOutArgs oa{};
        oa.cand_read = cand_read; oa.cand_locus = cand_locus; oa.row = ctx->d_pc_row; oa.is_row = is_row; oa.row_off = row_off; oa.ext = ctx->d_pc_ext; oa.ulen = d_ulen;
        oa.n_cand = (int32_t)Cn; oa.max_tail = max_tail;
        oa.out = { kept_col<int32_t>(k, PK_READ), kept_col<int32_t>(k, PK_LOCUS),
                   { kept_col<uint8_t>(k, PK_PARTIAL), kept_col<uint8_t>(k, PK_SLOT), kept_col<int32_t>(k, PK_FDIST), kept_col<int32_t>(k, PK_WINDOW), kept_col<int32_t>(k, PK_EXT),
                     kept_col<float>(k, PK_RATIO), kept_col<uint8_t>(k, PK_OPEN) } };
        hipLaunchKernelGGL(mtr_k_ptc_out, per_cand, b256, 0, ctx->stream, oa);
        HIPCHK(hipGetLastError());
    }
    *out_R = R;
    return MTR_OK;
}

extern "C" mtr_status mtr_test_partial_catalog_stats(mtr_ctx *ctx, int64_t *counts, double *ms)
{
    if (!ctx || !counts || !ms) return MTR_ERR_BAD_ARG;
    if (!ctx->pc.ready) { ctx->err = "no partial catalogue call to report on"; return MTR_ERR_BAD_ARG; }
    std::copy(ctx->pc.counts, ctx->pc.counts + 4, counts); std::copy(ctx->pc.ms, ctx->pc.ms + 3, ms);
    return MTR_OK;
}

extern "C" mtr_status mtr_genotype_partial_catalog_copy_device(mtr_ctx *ctx, const mtr_partial_catalog_dst *dst)
{
    if (!ctx) return MTR_ERR_BAD_ARG;
    if (!ctx->pc.ready) { ctx->err = "no rows kept: mtr_genotype_partial_catalog_device comes first (an upload discards what it kept)"; return MTR_ERR_BAD_ARG; }
    if (!dst) { ctx->err = "dst is NULL"; return MTR_ERR_BAD_ARG; }
    const mtr_partial_dst &g = dst->rows;
    void *const cols[CAT_ROW_COLS] = { dst->read, dst->locus, g.partial, g.slot, g.flank_dist, g.window, g.ext, g.ratio, g.open };      // the order of PK_*
    return kept_rows_copy(ctx, ctx->pc, ctx->d_pk, pk_row_bytes, cols, g.cap_rows);
}

// ---- the catalogue calls' entry points --------------------------------------------------------------------------------------------------
// What the four share: the arguments, the outputs zeroed, a pending run waited for, the kind's kept rows forgotten whatever happens after that.
// no_cat: a prepared call without its catalogue, refused before anything is waited for or forgotten.
static mtr_status catalog_call_begin(mtr_ctx *ctx, bool partial, bool no_cat, int64_t *out_rows, int64_t *out_candidates)
{
    if (!ctx || !out_rows || !out_candidates) return MTR_ERR_BAD_ARG;
    *out_rows = 0; *out_candidates = 0;
    if (no_cat) { ctx->err = "cat is NULL"; return MTR_ERR_BAD_ARG; }
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    (partial ? ctx->pc : ctx->gc).ready = false;
    return MTR_OK;
}
// a catalogue call of either kind from the index on, whoever made it (ix, cm): the front, the kind's middle, the tail
static mtr_status catalog_run(mtr_ctx *ctx, bool partial, const CatIndex &ix, const CatMotifs &cm, int32_t n_loci, int32_t max_flank_dist, int q, int32_t gain, int32_t mismatch,
                              int32_t indel, int32_t max_tail, double ms_index, int64_t *out_rows, int64_t *out_candidates)
{
    CatFront f; CatCandArgs gca{}; PtcCandArgs pca{};
    int64_t R = 0;
    mtr_status st = partial ? catalog_front(ctx, ix, q, "genotype_partial_catalog", "the partial catalogue's", mtr_k_ptc_cands, pca, f)
                            : catalog_front(ctx, ix, q, "genotype_catalog", "the catalogue's", mtr_k_cat_cands, gca, f);
    if (st == MTR_OK && f.Cn > 0)
        st = partial ? partial_catalog_rows(ctx, ix, cm, f, pca, n_loci, max_flank_dist, gain, mismatch, indel, max_tail, &R)
                     : genotype_catalog_rows(ctx, ix, cm, f, gca, n_loci, max_flank_dist, gain, mismatch, indel, &R);
    return st != MTR_OK ? st : catalog_finish(ctx, partial ? ctx->pc : ctx->gc, f, q, ms_index, R, out_rows, out_candidates);
}

// A text-taking call: the genotype's checks, then the kind's own (the DP's size, or the partial genotype's) and the seeds'; the switches; the
// index, timed on the host (its copies are synchronous); the run
static mtr_status catalog_text_call(mtr_ctx *ctx, bool partial, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist, int32_t seed_len,
                                    int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail, int64_t *out_rows, int64_t *out_candidates)
{
    { mtr_status st = catalog_call_begin(ctx, partial, false, out_rows, out_candidates); if (st != MTR_OK) return st; }
    LociText lt;
    { mtr_status st = genotype_check_args(ctx, seqs, seq_off, n_loci, max_flank_dist, gain, mismatch, indel, lt); if (st != MTR_OK) return st; }
    { mtr_status st = partial ? partial_check_args(ctx, lt.L.mot_off, n_loci, max_tail) : search_motifs_check_size(ctx, lt.L.mot_off.data(), n_loci); if (st != MTR_OK) return st; }
    LA_CHK(la_check_seeds(lt.L.plen, n_loci, max_flank_dist, seed_len, ctx->err));
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    const auto t_start = HostClock::now();
    CatIndex ix;
    { mtr_status st = catalog_index(ctx, lt.pat, max_flank_dist + 1, seed_len, ix); if (st != MTR_OK) return st; }
    const double ms_index = ms_since(t_start);
    const CatMotifs cm = { &lt.mot, &lt.L.mot_off, nullptr };
    return catalog_run(ctx, partial, ix, cm, n_loci, max_flank_dist, seed_len, gain, mismatch, indel, max_tail, ms_index, out_rows, out_candidates);
}

extern "C" mtr_status mtr_genotype_catalog_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist, int32_t seed_len,
                                                  int32_t gain, int32_t mismatch, int32_t indel, int64_t *out_rows, int64_t *out_candidates)
{
    return catalog_text_call(ctx, false, seqs, seq_off, n_loci, max_flank_dist, seed_len, gain, mismatch, indel, 0, out_rows, out_candidates);
}

extern "C" mtr_status mtr_genotype_partial_catalog_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist, int32_t seed_len,
                                                          int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail, int64_t *out_rows, int64_t *out_candidates)
{
    return catalog_text_call(ctx, true, seqs, seq_off, n_loci, max_flank_dist, seed_len, gain, mismatch, indel, max_tail, out_rows, out_candidates);
}

// ---- a prepared locus catalogue (catalog_build.hip.inc) ---------------------------------------------------------------------------------
// mtr_catalog_create: one pass over seq_off on the host (la_lengths: the first refused length, the slots' and the motifs' lengths and offsets),
// one upload of the letters and of those small arrays, the letters' check (a second look at the device: the first bad byte), then the build - the
// slots, the sort's passes (count, scan, fill), the flags and their two scans, a third look (the entries, the distinct codes: they size the
// catalogue's buffers), the compaction, the table, the motif tables - and the status.  The working buffers are freed when the call returns.
// The two prepared calls are the text-taking calls from the index on (catalog_run).
extern "C" mtr_status mtr_catalog_create(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist, int32_t seed_len, mtr_catalog **out)
{
    if (!ctx || !out) return MTR_ERR_BAD_ARG;
    *out = nullptr;
    if (end_pending_run(ctx) != MTR_OK) return MTR_ERR_HIP;
    const auto t_host = HostClock::now();
    // genotype_check_args' checks that need no batch, in its order; the device adds the first bad byte to the first bad length (catb_bad_key)
    LA_CHK(la_check_offsets(seqs, seq_off, n_loci, ctx->err));
    const size_t nl = (size_t)n_loci, S = nl * GT_SLOTS;
    LociLengths L;
    la_lengths(seq_off, n_loci, L);
    LA_CHK(la_check_motif_total(n_loci, L.mot_off[nl], ctx->err));
    std::unique_ptr<mtr_catalog> cat(new mtr_catalog);
    static std::atomic<uint64_t> next_id{ 1 };
    cat->id = next_id.fetch_add(1);
    cat->device = ctx->device; cat->n_loci = n_loci; cat->max_flank_dist = max_flank_dist; cat->seed_len = seed_len;
    cat->mot_off = L.mot_off; cat->unit_off = L.unit_off; cat->n_short = L.n_short; cat->n_long = L.n_long; cat->first_long_motif = L.first_long_motif;
    const int64_t n_bytes = L.off[3 * nl], units_at = L.unit_off[2 * nl];
    const double ms_host = ms_since(t_host);
    // the uploads, and the letters' check
    HIPCHK(hipSetDevice(ctx->device));
    const auto t_up = HostClock::now();
    DevBuf<char> w_seqs; DevBuf<int64_t> w_off; DevBuf<unsigned long long> w_bad; DevBuf<int32_t> w_status;
    HIPCHK(w_seqs.alloc((size_t)n_bytes + 16)); HIPCHK(w_off.alloc((3 * nl + 1) * 8)); HIPCHK(w_bad.alloc(8)); HIPCHK(w_status.alloc(4));
    HIPCHK(cat->d_plen.alloc(S * 4)); HIPCHK(cat->d_uoff.alloc((2 * nl + 1) * 4)); HIPCHK(cat->d_ulen.alloc(nl * 4));
    if (n_bytes > 0) HIPCHK(copy_sync(ctx, w_seqs, seqs + seq_off[0], (size_t)n_bytes, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, w_off, L.off.data(), (3 * nl + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, cat->d_plen, L.plen.data(), S * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, cat->d_uoff, L.unit_off.data(), (2 * nl + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_sync(ctx, cat->d_ulen, L.ulen.data(), nl * 4, hipMemcpyHostToDevice));
    const double ms_upload = ms_since(t_up);
    const auto t_build = HostClock::now();
    const CatbSrc src = { w_seqs, w_off, n_loci };
    const dim3 b64(64), b256(256), one(1), b1024(1024);
    HIPCHK(hipMemsetAsync(w_bad, 0xFF, 8, ctx->stream)); HIPCHK(hipMemsetAsync(w_status, 0, 4, ctx->stream));
    hipLaunchKernelGGL(mtr_k_catb_check, dim3((unsigned)((3 * nl + 255) / 256)), b256, 0, ctx->stream, src, (unsigned long long *)w_bad);
    HIPCHK(hipGetLastError());
    unsigned long long dev_bad = CATB_NO_BAD_BYTE;
    HIPCHK(copy_sync(ctx, &dev_bad, w_bad, 8, hipMemcpyDeviceToHost));
    const unsigned long long bad = std::min(L.first_bad_length, dev_bad);
    if (bad != LA_NO_KEY) {
        if (la_key_refusal(bad, seqs, seq_off, ctx->err)) return MTR_ERR_BAD_ARG;
        ctx->err = "the catalogue's check of the letters failed on the device"; return MTR_ERR_HIP;
    }
    LA_CHK(la_check_flank_dist(max_flank_dist, ctx->err) && la_check_seeds(L.plen, n_loci, max_flank_dist, seed_len, ctx->err));
    // the build.  ((max_flank_dist + 1) * seed_len <= 64 from here on: every flank has at most 64 bases)
    const int q = seed_len, seeds = max_flank_dist + 1;
    const int64_t E0 = (int64_t)S * seeds;
    if (E0 > (int64_t)INT32_MAX) { ctx->err = std::to_string(S) + " slots x " + std::to_string(seeds) + " seeds are more than 2^31 - 1 entries"; return MTR_ERR_OVERFLOW; }
    const size_t e0 = (size_t)E0;
    const int n_tiles = (int)((e0 + CB_TILE - 1) / CB_TILE);
    const size_t nh = (size_t)CB_DIGITS * (size_t)n_tiles;
    DevBuf<uint32_t> w_keys[2], w_rkey; DevBuf<int32_t> w_vals[2], w_hist, w_keep, w_head, w_rfirst; DevBuf<int64_t> w_first, w_keepoff, w_headoff;
    for (int k = 0; k < 2; k++) { HIPCHK(w_keys[k].alloc(e0 * 4)); HIPCHK(w_vals[k].alloc(e0 * 4)); }
    HIPCHK(w_hist.alloc(nh * 4)); HIPCHK(w_first.alloc((nh + 1) * 8)); HIPCHK(w_keep.alloc(e0 * 4)); HIPCHK(w_head.alloc(e0 * 4));
    HIPCHK(w_keepoff.alloc((e0 + 1) * 8)); HIPCHK(w_headoff.alloc((e0 + 1) * 8));
    HIPCHK(cat->d_masks.alloc(S * FL_MASKS * 8));
    const CatbSlotArgs sl = { src, cat->d_plen, q, seeds, cat->d_masks, w_keys[0], w_vals[0], w_status };
    hipLaunchKernelGGL(mtr_k_catb_slots, dim3((unsigned)((S + 63) / 64)), b64, 0, ctx->stream, sl);
    const int passes = cb_passes(q);
    for (int p = 0; p < passes; p++) {
        const int from = p & 1, to = from ^ 1;
        hipLaunchKernelGGL(mtr_k_catb_count, dim3((unsigned)n_tiles), b64, 0, ctx->stream, (const uint32_t *)w_keys[from], (long long)E0, p, n_tiles, (int32_t *)w_hist);
        hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)w_hist, (int64_t)nh, (int64_t *)w_first);
        const CatbFillArgs fa = { w_keys[from], w_vals[from], (long long)E0, p, n_tiles, w_first, w_keys[to], w_vals[to], w_status };
        hipLaunchKernelGGL(mtr_k_catb_fill, dim3((unsigned)n_tiles), b64, 0, ctx->stream, fa);
    }
    const uint32_t *s_keys = w_keys[passes & 1]; const int32_t *s_vals = w_vals[passes & 1];
    const dim3 per_entry((unsigned)((e0 + 255) / 256));
    hipLaunchKernelGGL(mtr_k_catb_flags, per_entry, b256, 0, ctx->stream, s_keys, s_vals, (long long)E0, (int32_t *)w_keep, (int32_t *)w_head);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)w_keep, E0, (int64_t *)w_keepoff);
    hipLaunchKernelGGL(mtr_k_scan_offsets<int32_t>, one, b1024, 0, ctx->stream, (const int32_t *)w_head, E0, (int64_t *)w_headoff);
    HIPCHK(hipGetLastError());
    int64_t E = 0, distinct = 0; int32_t dev = 0;
    HIPCHK(copy_sync(ctx, &E, (int64_t *)w_keepoff + e0, 8, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, &distinct, (int64_t *)w_headoff + e0, 8, hipMemcpyDeviceToHost));
    HIPCHK(copy_sync(ctx, &dev, w_status, 4, hipMemcpyDeviceToHost));
    if (dev != DEV_OK || distinct < 1 || distinct > E || E > E0) { ctx->err = "the catalogue's sort failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    cat->E = (size_t)E; cat->distinct = (size_t)distinct;
    cat->cap = cb_table_cap((uint64_t)distinct); cat->fbits = cb_filter_bits((uint64_t)distinct); cat->fwords = ((size_t)1 << cat->fbits) / 32;
    const size_t cap = cat->cap;
    HIPCHK(cat->d_filter.alloc(cat->fwords * 4)); HIPCHK(cat->d_key.alloc(cap * 4)); HIPCHK(cat->d_run.alloc(2 * cap * 4)); HIPCHK(cat->d_ent.alloc(cat->E * 4));
    HIPCHK(w_rkey.alloc(cat->distinct * 4)); HIPCHK(w_rfirst.alloc((cat->distinct + 1) * 4));
    HIPCHK(hipMemsetAsync(cat->d_filter, 0, cat->fwords * 4, ctx->stream)); HIPCHK(hipMemsetAsync(cat->d_key, 0, cap * 4, ctx->stream)); HIPCHK(hipMemsetAsync(cat->d_run, 0, 2 * cap * 4, ctx->stream));
    const CatbCompactArgs co = { s_keys, s_vals, (long long)E0, w_keep, w_head, w_keepoff, w_headoff, (long long)E, (long long)distinct, cat->d_ent, w_rkey, w_rfirst, w_status };
    hipLaunchKernelGGL(mtr_k_catb_compact, per_entry, b256, 0, ctx->stream, co);
    const CatbTableArgs ta = { w_rkey, w_rfirst, (long long)distinct, cat->d_filter, cat->fbits, cat->d_key, cat->d_run, cat->cap, w_status };
    hipLaunchKernelGGL(mtr_k_catb_table, dim3((unsigned)((cat->distinct + 255) / 256)), b256, 0, ctx->stream, ta);
    // the motif tables
    HIPCHK(cat->d_units.alloc((size_t)units_at + 16)); HIPCHK(cat->d_ubits.alloc(2 * nl * 8)); HIPCHK(cat->d_vbits.alloc(4 * nl * 8));
    const CatbMotifArgs ma = { src, cat->d_ulen, cat->d_uoff, cat->d_units, cat->d_ubits, cat->d_vbits, w_status };
    hipLaunchKernelGGL(mtr_k_catb_motifs, dim3((unsigned)((nl + 255) / 256)), b256, 0, ctx->stream, ma);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_sync(ctx, &dev, w_status, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (dev == CATB_ERR_TABLE_FULL) { ctx->err = "the seed table is full"; return MTR_ERR_HIP; }
    if (dev != DEV_OK) { ctx->err = "the catalogue's build failed on the device (status " + std::to_string(dev) + ")"; return MTR_ERR_HIP; }
    DBG("catalog_create: %zu entries of %zu codes, table of %u slots, filter of 2^%d bits, %zu device bytes", cat->E, cat->distinct, cat->cap, cat->fbits, cat->device_bytes());
    ctx->cb_ready = true; ctx->cb_ms[0] = ms_host; ctx->cb_ms[1] = ms_upload; ctx->cb_ms[2] = ms_since(t_build);
    *out = cat.release();
    return MTR_OK;
}

extern "C" void mtr_catalog_destroy(mtr_catalog *cat)
{
    if (!cat) return;
    (void)hipSetDevice(cat->device);
    delete cat;
}

extern "C" mtr_status mtr_catalog_info_get(const mtr_catalog *cat, mtr_catalog_info *info)
{
    if (!cat || !info) return MTR_ERR_BAD_ARG;
    info->n_loci = cat->n_loci; info->max_flank_dist = cat->max_flank_dist; info->seed_len = cat->seed_len; info->filter_bits = cat->fbits;
    info->entries = (int64_t)cat->E; info->distinct_codes = (int64_t)cat->distinct; info->table_slots = (int64_t)cat->cap;
    info->first_long_motif = cat->first_long_motif; info->device_bytes = (int64_t)cat->device_bytes();
    return MTR_OK;
}

extern "C" mtr_status mtr_test_catalog_build_stats(mtr_ctx *ctx, double *ms)
{
    if (!ctx || !ms) return MTR_ERR_BAD_ARG;
    if (!ctx->cb_ready) { ctx->err = "no mtr_catalog_create to report on"; return MTR_ERR_BAD_ARG; }
    std::copy(ctx->cb_ms, ctx->cb_ms + 3, ms);
    return MTR_OK;
}

// A prepared call: the checks that depend on the batch or the call, in the text-taking calls' order (the loci's own were mtr_catalog_create's);
// the switches; ix pointed into cat; the run
static mtr_status catalog_prepared_call(mtr_ctx *ctx, const mtr_catalog *cat, bool partial, int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail,
                                        int64_t *out_rows, int64_t *out_candidates)
{
    { mtr_status st = catalog_call_begin(ctx, partial, !cat, out_rows, out_candidates); if (st != MTR_OK) return st; }
    if (ctx->device != cat->device) { ctx->err = "the catalogue was built on device " + std::to_string(cat->device) + ", the context runs on device " + std::to_string(ctx->device); return MTR_ERR_BAD_ARG; }
    if (ctx->n_reads <= 0) { ctx->err = "no batch uploaded"; return MTR_ERR_BAD_ARG; }
    const int32_t n_loci = cat->n_loci;
    LA_CHK(la_check_hits(ctx->n_reads, n_loci, ctx->err) && la_check_pairs(ctx->n_reads, n_loci, ctx->err));
    if (!partial) { mtr_status st = search_motifs_check_size(ctx, cat->mot_off.data(), n_loci); if (st != MTR_OK) return st; }
    LA_CHK(la_check_scores(gain, mismatch, indel, ctx->err));
    if (partial) { mtr_status st = partial_check_args(ctx, cat->mot_off, n_loci, max_tail); if (st != MTR_OK) return st; }
    HIPCHK(hipSetDevice(ctx->device));
    read_switches(ctx->sw);
    { mtr_status st = catalog_scan_buffers(ctx); if (st != MTR_OK) return st; }
    CatIndex ix;
    ix.E = cat->E; ix.distinct = cat->distinct; ix.fwords = cat->fwords; ix.cap = cat->cap; ix.fbits = cat->fbits;
    ix.narrow = ctx->sw.flank_word != 64 && cat->n_short > 0; ix.wide = ctx->sw.flank_word == 64 || cat->n_long > 0;      // flank_is_wide over the slots' lengths
    ix.d_filter = cat->d_filter; ix.d_key = cat->d_key; ix.d_run = cat->d_run; ix.d_ent = cat->d_ent; ix.d_plen = cat->d_plen; ix.d_masks = cat->d_masks;
    const CatMotifs cm = { nullptr, nullptr, cat };
    return catalog_run(ctx, partial, ix, cm, n_loci, cat->max_flank_dist, cat->seed_len, gain, mismatch, indel, max_tail, 0.0, out_rows, out_candidates);
}

extern "C" mtr_status mtr_genotype_catalog_prepared_device(mtr_ctx *ctx, const mtr_catalog *cat, int32_t gain, int32_t mismatch, int32_t indel, int64_t *out_rows,
                                                           int64_t *out_candidates)
{
    return catalog_prepared_call(ctx, cat, false, gain, mismatch, indel, 0, out_rows, out_candidates);
}

extern "C" mtr_status mtr_genotype_partial_catalog_prepared_device(mtr_ctx *ctx, const mtr_catalog *cat, int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail,
                                                                   int64_t *out_rows, int64_t *out_candidates)
{
    return catalog_prepared_call(ctx, cat, true, gain, mismatch, indel, max_tail, out_rows, out_candidates);
}

extern "C" mtr_status mtr_test_catalog_dump(mtr_ctx *ctx, const mtr_catalog *cat, mtr_catalog_dump *out)
{
    if (!ctx || !cat || !out) return MTR_ERR_BAD_ARG;
    if (ctx->device != cat->device) { ctx->err = "the catalogue was built on device " + std::to_string(cat->device) + ", the context runs on device " + std::to_string(ctx->device); return MTR_ERR_BAD_ARG; }
    memset(out, 0, sizeof *out);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nl = (size_t)cat->n_loci, S = nl * GT_SLOTS, cap = cat->cap, ub = (size_t)cat->unit_off[2 * nl];
    const struct { const void *d; size_t bytes; } src[11] = {
        { cat->d_filter, cat->fwords * 4 }, { cat->d_key, cap * 4 }, { cat->d_run, 2 * cap * 4 }, { cat->d_ent, cat->E * 4 }, { cat->d_plen, S * 4 }, { cat->d_masks, S * FL_MASKS * 8 },
        { cat->d_units, ub }, { cat->d_uoff, (2 * nl + 1) * 4 }, { cat->d_ubits, 2 * nl * 8 }, { cat->d_vbits, 4 * nl * 8 }, { cat->d_ulen, nl * 4 } };
    std::unique_ptr<void, FreeDeleter> h[11];
    for (int k = 0; k < 11; k++) {
        h[k].reset(malloc(std::max<size_t>(src[k].bytes, 1)));
        if (!h[k]) { ctx->err = "out of host memory"; return MTR_ERR_OOM; }
        if (src[k].bytes > 0) HIPCHK(copy_sync(ctx, h[k].get(), src[k].d, src[k].bytes, hipMemcpyDeviceToHost));
    }
    out->filter_words = (int64_t)cat->fwords; out->table_slots = (int64_t)cap; out->entries = (int64_t)cat->E; out->n_slots = (int64_t)S; out->unit_bytes = (int64_t)ub; out->n_loci = cat->n_loci;
    out->filter = (uint32_t *)h[0].release(); out->key = (uint32_t *)h[1].release(); out->run = (int32_t *)h[2].release(); out->ent = (int32_t *)h[3].release();
    out->plen = (int32_t *)h[4].release(); out->masks = (uint64_t *)h[5].release(); out->units = (uint8_t *)h[6].release(); out->unit_off = (int32_t *)h[7].release();
    out->unit_bits = (uint64_t *)h[8].release(); out->variant_bits = (uint64_t *)h[9].release(); out->ulen = (int32_t *)h[10].release();
    return MTR_OK;
}
