/*
 * mtr_oracle — TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C, single-threaded CPU restatement of the per-read hot path of reference mTR
 * (handle_one_read.c:190-266 and everything below it) under the "isolated semantics" contract of
 * each read is processed as if it were the only read in its process.
 * It exists so that tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg can check /
 * time the HIP path on machines where /root/reference does not exist.  Nothing under mtr_amd/
 * may include, link or call it.
 *
 * Parity status: PINNED — checked line by line against the capture points G1/G3/G3p/G3r/G4/G5
 * recorded from the unmodified reference by oracle/ref_capture.c (tests/test_oracle_golden.py,
 * tests/golden/), and against the md5 fingerprints of SURVEY.md Appendix C.
 */
#ifndef MTR_ORACLE_H
#define MTR_ORACLE_H
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTRO_MAX_PERIOD 500          /* mTR.h:35 */
#define MTRO_MAX_INPUT_LENGTH 1000000 /* mTR.h:31 */

/* One candidate repeat = the 17 arguments of insert_an_alignment_into_set (mTR.h:151-168),
 * minus readID/inputLen which are per read. */
typedef struct {
    int32_t rep_start, rep_end, repeat_len, rep_period, num_freq_unit;
    int32_t num_matches, num_mismatches, num_insertions, num_deletions;
    int32_t kmer, match_gain, mismatch_penalty, indel_penalty;
    char    unit[MTRO_MAX_PERIOD * 2 + 4]; /* NUL-terminated; room for a unit the revision doubled */
    int32_t unit_score[MTRO_MAX_PERIOD];
} mtro_record;

/* per-read work counters (used for DESIGN.md's C_alg / B_alg and by bench.py) */
typedef struct {
    int64_t dp_calls, dp_cells, dp_rows, dp_max_cells;
    int64_t revise_dp_calls, revise_dp_cells;
    int64_t kmer_tables, kmer_lookups, searches_passing_maxfreq;
    int64_t ranges_candidate, ranges_executed, records;
    int64_t di_passes, di_positions;
} mtro_stats;

typedef struct mtro_ctx mtro_ctx;

mtro_ctx *mtro_create(int manhattan, float min_match_ratio);
void      mtro_destroy(mtro_ctx *);
/* capture stream in the JSONL format of oracle/ref_capture.c (NULL = off); level as there */
void      mtro_set_capture(mtro_ctx *, FILE *cap, int level);
/* on = the reference's behaviour on a multi-read file instead of isolated semantics: the reads must then be given
 * in file order (results of a read depend on the longer reads before it).  Checked against the reference run on
 * whole files (tests/test_oracle_golden.py, capture points G1..G4; stdout up to the heap-order chaining ties). */
void      mtro_set_file_order(mtro_ctx *, int on);
const mtro_stats *mtro_get_stats(const mtro_ctx *);
void      mtro_reset_stats(mtro_ctx *);

/* codes[0..L): 0..3 = A C G T.  Returns the number of records (insertion order) written to
 * *out (malloc'ed, caller frees with free()), or <0 on error. */
int mtro_process_read(mtro_ctx *, const char *read_id, const uint8_t *codes, int L, mtro_record **out);

/* chaining.cpp:243-363 with insertion-order ties: writes the indices of the records of the best
 * chain, in print order, to chain_idx (capacity n); returns the chain length. */
int mtro_chain(const mtro_record *recs, int n, int *chain_idx);

/* chaining.cpp:125-171 (+ wrap_around_DP.c:57-213 when print_alignment): prints one chain. */
void mtro_print_chain(FILE *fp, const char *read_id, int L, const uint8_t *codes, const mtro_record *recs,
                      const int *chain_idx, int n_chain, int print_alignment);

/* the same for the read the context processed last, printed from the context's own read buffer (file-order mode: a
 * repeat can end on org[L], a base an earlier read left there) */
void mtro_print_chain_of_last_read(mtro_ctx *, FILE *fp, const char *read_id, const mtro_record *recs,
                                   const int *chain_idx, int n_chain, int print_alignment);

/* stand-alone pieces, exported so that tests can drive the HIP kernels' building blocks */
typedef struct {
    int32_t rep_start, rep_end, repeat_len, num_freq_unit, num_matches, num_mismatches, num_insertions, num_deletions;
} mtro_dp_result;
/* wrap_around_DP_sub (wrap_around_DP.c:222-354) on codes[] with org[p>=L]=0 */
int mtro_wrap_dp(const uint8_t *codes, int L, int query_start, int query_end, const uint8_t *unit, int unit_len,
                 int G, int MM, int D, mtro_dp_result *res);
/* search_De_Bruijn_graph (consensus.c:507-582) for ONE (window, k) of a read under isolated semantics: the found flag
 * (that of the last walk) and the record as capture point G2 shows it - every field -1 where no walk's unit
 * passed the selection; unit = "" unless 0 < period < MTRO_MAX_PERIOD.  Also what the search started from: the window's
 * maximum node count (no walk is made unless it exceeds 5, :532) and the seeds in the order they are tried.
 * Returns found, or <0 on bad arguments (or a file-order context). */
typedef struct {
    int32_t found, period, rep_start, rep_end, repeat_len, copies, mat, mis, ins, del;
    int32_t max_freq, n_seeds, seeds[100];
    char    unit[MTRO_MAX_PERIOD + 4];
} mtro_search_result;
int mtro_search_unit(mtro_ctx *, const uint8_t *codes, int L, int query_start, int query_end, int k, mtro_search_result *out);
/* one greedy walk (consensus.c:269-505) from `seed` on the same table, forward or backward: *out_period = the unit's
 * length, 0 if the walk does not return to the seed (or only after MTRO_MAX_PERIOD steps); out_unit (MTRO_MAX_PERIOD + 1
 * characters) = the unit, "" if none.  Returns 1 if the walk closed, 0 if not, <0 on bad arguments. */
int mtro_walk(mtro_ctx *, const uint8_t *codes, int L, int query_start, int query_end, int k, int backward, int seed,
              int *out_period, char *out_unit);
/* revise_representative_unit (consensus.c:1048-1087) for ONE record of a read under isolated semantics: polish_repeat (do_polish != 0; 0: the unit
 * given is already polished, as the staged chain hands it to its revision kernel), then the two rounds (vote DP (5,1,1) / (1,1,3), revised unit,
 * re-alignment, acceptance against the ratio the revision started with) - through the statics mtro_process_read runs, so what a test
 * learns here holds for a whole read.  in: the 13 scalar fields of the record, the unit's codes (0..3) and its node frequencies.  out: the final
 * record and unit, the polished unit's length, and per round what revise_representative_unit_sub was given (the fields of capture point G3r), the
 * threshold of the missing-base votes (min_missing; -1 where the coverage is outside 5..20), the revised unit, whether the votes left the unit as it
 * was, whether a candidate was made (0 < revised length < MTRO_MAX_PERIOD), whether it was accepted and whether that moved rep_start or rep_end.
 * Leaves no capture line.  Returns 0, or < 0 and nothing done: a file-order context or a bad read (-1); a period outside 1..499 or unit_len that
 * differs from it (-2); a window outside 0 <= rep_start <= rep_end <= L (-3; rep_end = L is what a repeat that runs to the end of its read gives,
 * org[L..L+3] = 0); mat + mis + ins + del <= 0, a negative count or repeat_len <= 0 (-4); k outside 1..15 (-5); (2 period + 1) rows + 2
 * period >= WrapDPsize, where a round's DP of a revised unit could end the process (-6); a unit code above 3 (-7). */
typedef struct {
    int32_t rep_start, rep_end, repeat_len, rep_period, copies, mat, mis, ins, del, kmer, G, MM, D;
    int32_t unit_len;
    uint8_t unit[MTRO_MAX_PERIOD];
    int32_t score[MTRO_MAX_PERIOD];
} mtro_revise_in;
typedef struct {
    int32_t in_start, in_end, in_repeat_len, in_mis, in_ins, in_del, in_len, threshold;
    int32_t rev_len, unchanged, candidate, accepted, moved;
    uint8_t in_unit[MTRO_MAX_PERIOD], rev_unit[MTRO_MAX_PERIOD * 2 + 4];
} mtro_revise_round;
typedef struct {
    int32_t rep_start, rep_end, repeat_len, rep_period, copies, mat, mis, ins, del, kmer, G, MM, D;
    int32_t polished_len;
    uint8_t unit[MTRO_MAX_PERIOD * 2 + 4];
    mtro_revise_round round[2];
} mtro_revise_out;
int mtro_revise(mtro_ctx *, const uint8_t *codes, int L, const mtro_revise_in *in, int do_polish, mtro_revise_out *out);
/* fill_directional_index_with_end (+ de-dup); arrays of length L; returns number of usable ranges */
int mtro_ranges(mtro_ctx *, const uint8_t *codes, int L, double *di, int32_t *end, int32_t *w);
/* the same, and (either may be NULL) end_raw[i] = the end of the entry at i BEFORE the de-duplication, k_raw[i] = the k of the pass that
 * recorded it (-1: no entry): the list the de-duplication chain walks and the pass (k, w) of every entry, for tests that choose reads by them */
int mtro_ranges_raw(mtro_ctx *, const uint8_t *codes, int L, double *di, int32_t *end, int32_t *w, int32_t *end_raw, int32_t *k_raw);
/* the MT19937 stream (MT.h) after init_genrand(0): out[i] = genrand_int32() % 4 */
void mtro_mt_bases(uint8_t *out, int n);

/* FASTA reader with the reference's quirks (handle_one_file.c:201-269).  Returns number of reads;
 * ids[i], seqs[i] (codes 0..3), lens[i] are malloc'ed.  Exits like the reference on a bad character. */
int mtro_read_fasta(const char *path, char ***ids, uint8_t ***seqs, int **lens);

#ifdef __cplusplus
}
#endif
#endif
