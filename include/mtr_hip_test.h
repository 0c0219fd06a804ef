/*
 * mtr_hip_test.h — entry points of libmtr_hip.so that exist for parity tests and debugging only (the same kernels the
 * batch path of include/mtr_hip.h runs, reachable stage by stage).  Not part of the drop-in boundary: a maintainer of
 * the reference binds include/mtr_hip.h alone.
 */
#ifndef MTR_HIP_TEST_H
#define MTR_HIP_TEST_H

#include "mtr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K1 alone = fill_directional_index_with_end (fill_directional_index.c:549-602) for every read of the
 * uploaded batch.  Returns per read the surviving candidate ranges (start ascending): start, end, w
 * and the DI value's IEEE-754 bit pattern.  Arrays are malloc'ed; free() them. */
mtr_status mtr_test_ranges(mtr_ctx *ctx, int32_t **out_counts, int32_t **out_start, int32_t **out_end,
                           int32_t **out_w, uint64_t **out_di_bits, int64_t *out_total);

/* The same ranges from the range finder's OTHER arrangement: the three kernels the staged chain launches for a batch of few reads
 * (launch_k1_parts: the code arrays; one work item per (read, pass, position segment); extraction as a pipeline of 16 wavefronts per
 * read, compaction and de-duplication by the workgroup), run alone on the resident batch over per-read scratch of n_reads *
 * k1_layout(Lmax).total bytes - exactly as launch_staged reaches them.  Outputs and malloc'ed arrays as mtr_test_ranges.
 *   mode     follows the resident batch: uploaded with a file state (mtr_upload_batch_in_file and the device uploads in a file), the passes
 *            run whole and the finish is one wavefront per read; any other batch has its passes cut into segments and the pipeline finish.
 *            The context's DI (Manhattan / Pearson) selects the passes.
 *   refused  with MTR_ERR_BAD_ARG and a reason, nothing launched: no resident batch; more than 256 reads; per-read scratch for every read
 *            that does not fit the context's scratch budget (MTR_SCRATCH_MAX_GB, free memory) - the batches launch_staged hands to the
 *            one-wavefront-per-read kernel instead.
 * Status and counters are cleared first; afterwards id 0 of mtr_get_kernel_times is the time between two events of the entry's own
 * around the launches (launches = 3, or 2 where no read has a pass), and the context runs the batch as before (mtr_run_resident). */
mtr_status mtr_test_ranges_parts(mtr_ctx *ctx, int32_t **out_counts, int32_t **out_start, int32_t **out_end,
                                 int32_t **out_w, uint64_t **out_di_bits, int64_t *out_total);

/* wrap_around_DP_sub (wrap_around_DP.c:222-354) for n_tasks (read, window, unit, scores) tasks on the
 * uploaded batch.  unit codes 0..3, units concatenated, unit_off[n_tasks+1].  out8[8*t..] =
 * rep_start, rep_end, repeat_len, Num_freq_unit, matches, mismatches, insertions, deletions. */
mtr_status mtr_test_wrap_dp(mtr_ctx *ctx, int32_t n_tasks, const int32_t *read_idx, const int32_t *query_start,
                            const int32_t *query_end, const uint8_t *units, const int32_t *unit_off,
                            const int32_t *gain, const int32_t *mismatch, const int32_t *indel, int32_t *out8);

/* ONE chosen forward pass of the wrap-around DP, with its tracebacks, on groups the caller chose: group g = tasks group_off[g] .. group_off[g + 1]
 * (group_off[0] = 0, group_off[n_groups] = the number of tasks), the DPs that share one forward pass.  The task arrays are mtr_test_wrap_dp's.
 * out16[16 t + 8 p ..] = the eight integers of mtr_test_wrap_dp for task t and parameter set p, same window convention (row i is base
 * query_start + i).  The two-parameter passes ignore gain / mismatch / indel: p = 0 is (1,1,3), p = 1 is (1,3,1).  The one-parameter passes
 * take the task's own set, one of (1,1,3), (1,3,1), (5,1,1), and fill p = 0 only (p = 1: zeros).
 *   MTR_TEST_PASS_WAVE2P  groups of 1 task: dp_wrap2 where dp_wrap2_fits, else dp_wrap twice (dp_two_params_unit's decision)
 *   MTR_TEST_PASS_Q4      1-4 units of at most 16 bases over the same read and window: dp_forward2p_q4 + tracebacks, under dp_batch_fits
 *   MTR_TEST_PASS_QUAD2P  1-4 tasks of one DPQ_COLS class: the forward pass and tracebacks of mtr_k_dp2_quads (units <= 128, DPQ_FITS(rows, U, 1, 3))
 *   MTR_TEST_PASS_FOUR1P  1-4 tasks: a pass of mtr_k_revise_quads with one DP per 16 lanes, at the widest member's width, + counting tracebacks
 *   MTR_TEST_PASS_OCT1P   1-8 tasks: the same with two DPs per 16 lanes; member d is half d & 1 of lane group d >> 1
 *   MTR_TEST_PASS_OCT2P   1-8 tasks of units of at most 32 bases: the forward pass and tracebacks of mtr_k_dp2_quads' eight-per-wavefront part, at
 *                         ceil(longest unit / 8) columns per lane (DPQ_FITS(rows, U, 1, 3)); member d is lanes 8 d .. 8 d + 7
 * A task the batch path would never hand to the pass (the same bounds: units, rows, 16-bit scores, WrapDPsize), a group of another size, members of
 * QUAD2P classes or Q4 windows that differ, a window outside its read: MTR_ERR_BAD_ARG, the reason names the task; nothing is launched.
 * The entry sizes its own cell scratch from the passes' block macros, so the batch path's "the block fits this launch's cell budget" terms
 * (dp_batch_fits' 4 x 16 x rows, DPQ_BLOCK_BYTES / DPQP_BLOCK_BYTES against the cells of a batch) are held against the context's scratch cap
 * (MTR_SCRATCH_MAX_GB) instead: a group whose block exceeds it is refused in the same way. */
enum { MTR_TEST_PASS_WAVE2P = 0, MTR_TEST_PASS_Q4 = 1, MTR_TEST_PASS_QUAD2P = 2, MTR_TEST_PASS_FOUR1P = 3, MTR_TEST_PASS_OCT1P = 4, MTR_TEST_PASS_OCT2P = 5 };
mtr_status mtr_test_wrap_dp_pass(mtr_ctx *ctx, int32_t pass, int32_t n_groups, const int32_t *group_off, const int32_t *read_idx,
                                 const int32_t *query_start, const int32_t *query_end, const uint8_t *units, const int32_t *unit_off,
                                 const int32_t *gain, const int32_t *mismatch, const int32_t *indel, int32_t *out16);

/* polish_repeat (consensus.c:610-704) alone, through the function the kernels run (polish(), k2_units.hip.inc), one wavefront per task, on the
 * uploaded batch.  Task t: the repeat rep_start[t] .. rep_end[t] (0-origin, inclusive) of read read_idx[t], k[t] (2 .. 15), the unit
 * units[unit_off[t] .. unit_off[t+1]) (codes 0..3, fewer than 500 bases) and its node frequencies scores[unit_off[t] ..] (unit_off has
 * n_tasks + 1 entries and starts at 0).  out_len[t] = the polished unit's length, its codes at out_units[500 t ..] (the caller's
 * 500 n_tasks bytes).  A task outside these bounds: MTR_ERR_BAD_ARG, the reason names it; nothing is launched. */
mtr_status mtr_test_polish(mtr_ctx *ctx, int32_t n_tasks, const int32_t *read_idx, const int32_t *rep_start, const int32_t *rep_end,
                           const int32_t *k, const uint8_t *units, const int32_t *scores, const int32_t *unit_off,
                           uint8_t *out_units, int32_t *out_len);

/* revise_representative_unit (consensus.c:1048-1087) on records and units of the caller's choosing, on the uploaded batch.  Task t: read read_idx[t], the 13
 * scalar fields of its record rr[13 t ..] in the order of mtr_record (rep_start, rep_end, repeat_len, rep_period, num_freq_unit, matches, mismatches,
 * insertions, deletions, kmer, match_gain, mismatch_penalty, indel_penalty), the unit units[unit_off[t] .. unit_off[t+1]) (codes 0..3; its length is the
 * record's period) and its node frequencies scores[unit_off[t] ..].  Group g = tasks group_off[g] .. group_off[g + 1] (group_off[0] = unit_off[0] = 0).
 * out_rr[13 t ..] = the record after the revision, out_units[500 t ..] its unit (rep_period codes; the caller's 500 x tasks bytes).
 *   MTR_TEST_REVISE_WAVE   a test kernel with mtr_k_revise's arena and launch bounds: the tasks of a group go through revise() - polish_repeat first - one after
 *                          the other on one wavefront, as the per-read path runs the k of a range; the round memo starts empty with the group and lives across
 *                          its tasks.  waves: a bound on the grid (0: none).
 *   MTR_TEST_REVISE_SLOTS  mtr_k_revise_quads ITSELF on `waves` wavefronts (0: one) over a work list built from the tasks in the order given (the groups only
 *                          cut the list for the reasons' sake): which revisions share a wavefront's eight slots follows from that order, and with one wavefront
 *                          from nothing else.  The unit given is the POLISHED one (the chain polishes in mtr_k_polish); the node frequencies travel along.
 *                          MTR_DP16_MAX_ROWS applies as in a batch run.
 * Scratch per wavefront and the cell budget are those launch_staged gives the kernels for the resident batch; *out_cells = that budget (k2_layout's cells:
 * what decides whether a pass's block fits).  The context's counters are cleared first and describe this launch afterwards (mtr_get_counters).
 * Refused with MTR_ERR_BAD_ARG, the reason naming task and group, nothing launched - what the batch path never hands to a revision (mtr_amd/csrc/revise_task.h):
 * a period outside 6..499 or a unit of another length; repeat_len / period outside 5..20; a window outside 0 <= rep_start <= rep_end <= L (rep_end = L is
 * taken: a repeat that runs to the end of its read); a negative count, matches + mismatches + insertions + deletions <= 0 or repeat_len <= 0; kmer outside
 * 2..15; (2 period + 1) rows + 2 period >= WrapDPsize; a unit code above 3; no resident batch; no group or an empty one; more than 4096 tasks; WAVE: a
 * group whose tasks lie in different reads (the round memo is a range's: its key does not hold the read).
 * Afterwards the context runs the batch as before (mtr_run_resident). */
enum { MTR_TEST_REVISE_WAVE = 0, MTR_TEST_REVISE_SLOTS = 1 };
mtr_status mtr_test_revise(mtr_ctx *ctx, int32_t mode, int32_t n_groups, const int32_t *group_off, const int32_t *read_idx, const int32_t *rr,
                           const uint8_t *units, const int32_t *scores, const int32_t *unit_off, int32_t waves, int32_t *out_rr, uint8_t *out_units,
                           int64_t *out_cells);

/* How the last launch ran: 0 = one kernel, a wavefront per read; 1 = range-parallel; 2 = the staged chain of kernels.
 * (The records do not depend on it; tests pin the policy of mtr_hip.h's mtr_set_overlapped_launches with it.) */
int32_t mtr_test_last_mode(const mtr_ctx *ctx);

/* Event trace of the last run (debug aid for parity work): enable before mtr_run_resident.
 * Each event is 16 int32: [0]=type (2 search, 3 DP, 4 polish, 5 revise, 6 record, 7 per-read cost, 8 per-walk cost), [1]=read index,
 * then type-specific fields (the trace_ev() calls in mtr_amd/csrc/k2_units.hip.inc). */
mtr_status mtr_set_trace(mtr_ctx *ctx, int32_t max_events);
mtr_status mtr_get_trace(mtr_ctx *ctx, int32_t **out_events, int64_t *out_n);

/* The chain kernel of mtr_report_device on caller-given records: set k is (start, end, matches)[set_off[k] .. set_off[k+1])
 * (set_off has n_sets + 1 entries, set_off[0] = 0).  (*out_len)[k] = its chain's length, the chain (indices within the set, print
 * order) at (*out_idx)[set_off[k] ..].  Both arrays are malloc'ed; free() them. */
mtr_status mtr_test_chain(mtr_ctx *ctx, int32_t n_sets, const int64_t *set_off, const int32_t *start, const int32_t *end,
                          const int32_t *matches, int32_t **out_len, int32_t **out_idx);

/* The line function of mtr_report_text_device on caller-given rows (the counterpart of mtr_test_chain).  Row k: the 14 header ints
 * fields[14k ..], its read's length read_len[k], the unit bytes units[unit_off[k] .. unit_off[k+1]) printed as they are, and the ID
 * ids[id_off[k] .. id_off[k+1]); unit_off and id_off have n_rows + 1 entries and start at 0.  Row k's line is
 * (*out_text)[(*out_off)[k] .. (*out_off)[k+1]).  Both arrays are malloc'ed; free() them. */
mtr_status mtr_test_report_lines(mtr_ctx *ctx, int32_t n_rows, const int32_t *fields, const int32_t *read_len, const uint8_t *units,
                                 const int64_t *unit_off, const char *ids, const int64_t *id_off, uint8_t **out_text, int64_t **out_off);

/* What the last successful mtr_genotype_catalog_device call of the context saw: counts[4] = the reads' seed positions, those the filter let
 * through, the seed hits, the candidates; ms[3] = host clock over the host's index build and upload, the first scan pass up to the look that ends
 * it, and the rest of the call.  For tests/dev/gpu_catalog.py.  MTR_ERR_BAD_ARG without such a call. */
mtr_status mtr_test_catalog_stats(mtr_ctx *ctx, int64_t *counts, double *ms);

/* The same of the last successful mtr_genotype_partial_catalog_device call of the context (its candidates are (read, locus) pairs).  For
 * tests/dev/gpu_partial_catalog.py.  MTR_ERR_BAD_ARG without such a call. */
mtr_status mtr_test_partial_catalog_stats(mtr_ctx *ctx, int64_t *counts, double *ms);

/* Host copies of everything a prepared catalogue holds on the device (tests/test_gpu_catalog_prepared.py).  ctx: a context on the catalogue's
 * device (its stream makes the copies).  Every array is malloc'ed, free() them; on anything but MTR_OK none is.
 *   filter [filter_words]   key [table_slots]   run [table_slots][2] (first, count; count = 0: empty)   ent [entries]
 *   plen [n_slots]   masks [n_slots][8]   (n_slots = 4 * n_loci)
 *   units [unit_bytes]   unit_off [2 * n_loci + 1]   unit_bits [2 * n_loci]   variant_bits [4 * n_loci]   ulen [n_loci] */
typedef struct mtr_catalog_dump {
    int64_t filter_words, table_slots, entries, n_slots, unit_bytes, n_loci;
    uint32_t *filter, *key;
    int32_t *run, *ent, *plen;
    uint64_t *masks;
    uint8_t *units;
    int32_t *unit_off;
    uint64_t *unit_bits, *variant_bits;
    int32_t *ulen;
} mtr_catalog_dump;
mtr_status mtr_test_catalog_dump(mtr_ctx *ctx, const mtr_catalog *cat, mtr_catalog_dump *out);
/* ms[3] of the last successful mtr_catalog_create on ctx, by the host clock: the host's pass over seq_off, the uploads (seqs and the length
 * arrays), the device build up to the synchronisation that ends it.  For tests/dev/gpu_catalog_prepared.py.  MTR_ERR_BAD_ARG without one. */
mtr_status mtr_test_catalog_build_stats(mtr_ctx *ctx, double *ms);

/* The kernels of mtr_report_motifs_device on caller-given units (the counterpart of mtr_test_chain).  Unit k is units[unit_off[k] ..
 * unit_off[k+1]) (unit_off has n + 1 entries and starts at 0), a repeat of read read[k] with num_freq_unit copies[k] and repeat_len[k].
 * A byte outside ACGT, a unit longer than 500, a decreasing read: MTR_ERR_BAD_ARG.  table_slots sizes the grouping's table so that a small
 * input can fill it (n = 1000 units with table_slots = 1024 walk long probe sequences).  The per-unit arrays have n entries, the per-group
 * arrays *out_groups, motif_off one more; all are malloc'ed, free() them.  A resident batch's catalogue is made again on its next use. */
mtr_status mtr_test_unit_motifs(mtr_ctx *ctx, int32_t n, const char *units, const int64_t *unit_off, const int32_t *read /* non-decreasing */,
                                const int32_t *copies, const int32_t *repeat_len, int64_t table_slots /* 0: the product's choice; else a power of two > n */,
                                /* malloc'ed, free() them: */ uint8_t **strand, int32_t **rotation, int32_t **motif_len, int32_t **group,
                                int64_t *out_groups, int64_t **motif_off, uint8_t **motifs, int32_t **g_first, int32_t **g_repeats, int32_t **g_reads,
                                int64_t **g_copies, int64_t **g_bases);

/* What file-order mode gave the resident batch, after a host (mtr_upload_batch_in_file) or a device (mtr_upload_batch_device_in_file,
 * mtr_upload_fasta_device_in_file) upload: read i's stale entries of inputString_w_rand are (*out_tail)[(*out_tail_off)[i] ..
 * (*out_tail_off)[i + 1]) (out_tail_off has n_reads + 1 entries), its orgInputString[L], [L + 1] are (*out_after)[2i], [2i + 1].
 * After an isolated upload: empty tails and zeros.  The arrays are malloc'ed; free() them.  Afterwards id 0 of
 * mtr_get_kernel_times is the tail kernel (mtr_k_file_tail) of that upload: launches = 0 after a host upload or with no entry. */
mtr_status mtr_test_file_tail(mtr_ctx *ctx, uint16_t **out_tail, int64_t **out_tail_off, uint8_t **out_after);

/* The rounds the last successful mtr_window_edits_device call of the context took (0: no window had a DP).  MTR_TEST_WE_SCRATCH_BYTES=<bytes>,
 * read per call, replaces MTR_WE_SCRATCH_BYTES as the cap on a round's stored decisions, so that small windows take several rounds; the edits do
 * not depend on it.  MTR_ERR_BAD_ARG without such a call. */
mtr_status mtr_test_window_edits_rounds(mtr_ctx *ctx, int32_t *rounds);

/* Environment switches for tests, read once per launch next to MTR_TEST_STAGED_CAPS and MTR_TEST_STAGED_FLAGS (read_switches, mtr_abi.hip):
 *   MTR_TEST_WALK_SCREEN=0   the staged chain without its dead-range screen (mtr_k_walk_screen): every candidate range is an item of mtr_k_walks,
 *                            as before the screen existed.  Records and counters do not depend on it.  (A traced run, mtr_set_trace, never screens.)
 *   MTR_TEST_STAGED_CAPS     also takes walk=<n>: the capacity of the list of ranges the screen leaves to mtr_k_walks (overflow: the per-read kernel
 *                            takes the batch, like any other list of the chain).
 *   MTR_TEST_MOTIF_LANE_MAX=<u>   mtr_search_motifs_device, read per call: the longest motif its lane path (one DP per lane, mtr_k_motif_lanes) takes,
 *                            0 .. 32; 0 sends every alignment through the wave path (mtr_k_motif_waves, one DP per wavefront).  The hits do not depend on it.
 *   MTR_TEST_MOTIF_LANE_ROWS=<n>  the longest read the lane path takes (at most its built-in bound of 16384 rows); longer reads take the wave path,
 *                            reads either side of the bound come from different kernels in one call.  The hits do not depend on it.
 *                            mtr_search_motif_loci_device reads both per call as well; there the bound on the rows is on the WINDOW's length, so the
 *                            short children of a long read are lanes' work.  The loci do not depend on either. */

#ifdef __cplusplus
}
#endif
#endif /* MTR_HIP_TEST_H */
