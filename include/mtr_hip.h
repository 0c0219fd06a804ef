/*
 * mtr_hip.h — C-ABI of libmtr_hip.so, the MI355X (gfx950) implementation of reference mTR's
 * per-read hot path.
 *
 * The reference has no FFI; the seam this library stands behind is the function boundary of its
 * per-read layer:
 *
 *   upper edge  void handle_one_read(char *readID, int inputLen, int read_cnt, int print_alignment)
 *               (reference mTR.h:127, called from handle_one_file.c:286), whose inputs also arrive
 *               through the globals orgInputString (mTR.h:65), Manhattan_Distance (mTR.h:61, -p sets
 *               it to 0) and min_match_ratio (mTR.h:62, -m);
 *   lower edge  insert_an_alignment_into_set(...17 arguments...) (mTR.h:151-168), called once per
 *               qualified repeat in candidate order (handle_one_read.c:156-176, :239-243).
 *
 * mtr_process_batch() is the batch form of that edge: it takes N reads as integer base codes
 * (what handle_one_file.c:284-285 copies into orgInputString) and returns, per read and in the
 * reference's insertion order, exactly the 17 arguments of insert_an_alignment_into_set (readID and
 * inputLen are the caller's own).  Printing (chaining.cpp) stays on the host side of the boundary
 * (mtr_amd/host/).  Chaining is done there too for the command line; mtr_report_device() makes the same chains on the
 * device for a caller that wants mTR's report without a host round trip.
 *
 * Semantics = the reference run one read per process ("isolated semantics"): the
 * results do not depend on which other reads share the batch.
 *
 * Conventions: every entry point returns an mtr_status; nothing calls exit(); the context owns all
 * device memory; one context per GPU / host thread; not re-entrant on one context.
 * There is NO CPU fallback: without a HIP device every entry point fails with MTR_ERR_NO_DEVICE.
 */
#ifndef MTR_HIP_H
#define MTR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_MAX_PERIOD 500          /* reference mTR.h:35 MAX_PERIOD */
#define MTR_MAX_INPUT_LENGTH 1000000 /* reference mTR.h:31: the reader's limit (a read that reaches it is fatal) */
/* Longest read the hot path takes: the reference's buffers hold L + 2r entries with r = L/10 random flank bases
 * (handle_one_read.c:194-204), so beyond L + 2r = MAX_INPUT_LENGTH it writes out of bounds; uploads refuse such reads. */
#define MTR_MAX_READ_LENGTH 833333
#define MTR_ABI_VERSION 5

typedef enum {
    MTR_OK = 0,
    MTR_ERR_NO_DEVICE = 1,      /* no HIP device / HIP runtime error at create */
    MTR_ERR_BAD_ARG = 2,        /* null pointer, bad length (<=0 or > MTR_MAX_READ_LENGTH), bad code (>3) */
    MTR_ERR_OOM = 3,            /* host or device allocation failed */
    MTR_ERR_HIP = 4,            /* a HIP call failed; mtr_last_error() has the text */
    MTR_ERR_OVERFLOW = 5,       /* a read produced more candidate ranges than L/2+64, or a caller-owned destination is too small */
    MTR_ERR_DP_TOO_LARGE = 6    /* a DP exceeded the reference's WrapDPsize (mTR.h:51): the reference exits */
} mtr_status;

/* One qualified repeat = arguments 3..17 of insert_an_alignment_into_set (mTR.h:151-168). */
typedef struct mtr_record {
    int32_t rep_start;          /* 0-origin, inclusive */
    int32_t rep_end;            /* 0-origin, inclusive */
    int32_t repeat_len;
    int32_t rep_period;
    int32_t num_freq_unit;
    int32_t num_matches;
    int32_t num_mismatches;
    int32_t num_insertions;
    int32_t num_deletions;
    int32_t kmer;
    int32_t match_gain;
    int32_t mismatch_penalty;
    int32_t indel_penalty;
    int32_t reserved;
    char    unit[MTR_MAX_PERIOD + 4];        /* "string", NUL-terminated ACGT */
    int32_t unit_score[MTR_MAX_PERIOD];      /* "string_score", first rep_period entries valid */
} mtr_record;

typedef struct mtr_ctx mtr_ctx;

/* device: HIP device ordinal.  manhattan: 1 = Manhattan DI (default), 0 = Pearson (-p).
 * min_match_ratio: the -m value (reference default 0.6, MIN_MATCH_RATIO mTR.h:32). */
mtr_status mtr_create(int device, int manhattan, float min_match_ratio, mtr_ctx **out);
void       mtr_destroy(mtr_ctx *ctx);
const char *mtr_last_error(const mtr_ctx *ctx);
int        mtr_abi_version(void);

/* Replaces the per-read loop body of handle_one_file.c:281-287 for n_reads reads at once.
 *   bases    concatenated base codes, one byte per base, 0..3 = A C G T (handle_one_file.c:169-188)
 *   offsets  n_reads start offsets into bases
 *   lens     n_reads lengths (1..MTR_MAX_READ_LENGTH)
 * On success *out_records is a malloc'ed array of all records, read after read, each read's records
 * in insertion order; (*out_counts)[i] is the number of records of read i.  Free both with
 * mtr_free_results(). */
mtr_status mtr_process_batch(mtr_ctx *ctx, const uint8_t *bases, const int64_t *offsets, const int32_t *lens,
                             int32_t n_reads, mtr_record **out_records, int32_t **out_counts, int64_t *out_total);
void       mtr_free_results(mtr_record *records, int32_t *counts);

/* The same path split so that a caller (bench.py) can keep inputs resident in HBM and time only the
 * device work: upload packs the reads to 2 bit/base and copies them to the device; run launches the
 * kernels on the context's stream and returns after they finish; fetch copies the records back. */
mtr_status mtr_upload_batch(mtr_ctx *ctx, const uint8_t *bases, const int64_t *offsets, const int32_t *lens, int32_t n_reads);
mtr_status mtr_run_resident(mtr_ctx *ctx);
/* The run split in two: _async enqueues the kernels on the context's stream and returns; mtr_wait blocks until
 * they finish and collects status, kernel times and counters.  Two contexts on one GPU can so overlap the tail of
 * one batch with the start of the next (bench.py pipelines its steps this way). */
mtr_status mtr_run_resident_async(mtr_ctx *ctx);
mtr_status mtr_wait(mtr_ctx *ctx);
mtr_status mtr_fetch_results(mtr_ctx *ctx, mtr_record **out_records, int32_t **out_counts, int64_t *out_total);

/* A failed run (mtr_wait returned an error) is remembered: fetch / export / alignments of that batch return the same
 * status instead of partial records.  After MTR_ERR_DP_TOO_LARGE the reads BEFORE the failing one (input order) are
 * still valid — the reference has printed them when it exits (wrap_around_DP.c:96-99) — and can be fetched with
 * mtr_fetch_results_packed(); *out_first_failed is the index of the first read whose DP exceeded WrapDPsize, or -1. */
mtr_status mtr_get_first_failed_read(const mtr_ctx *ctx, int32_t *out_first_failed);

/* ---- the host's own packing --------------------------------------------------------------------------------------
 * mtr_upload_batch packs the reads to the device layout on the calling thread.  A host that parses FASTA on several
 * threads packs there instead and hands over the finished image:
 *   read i occupies mtr_packed_words(lens[i]) = lens[i]/16 + 4 consecutive 32-bit words starting at word woff[i];
 *   base p of the read sits in word p>>4 at bits 31-2(p&15) .. 30-2(p&15) (first base in the top bits); every other
 *   bit of the read's words is 0 (org[L], org[L+1] read as 'A': isolated semantics).
 * mtr_pack_read writes one read's words (inline: a host needs no library for it); MTR_ERR_BAD_ARG for a code > 3. */
static inline int64_t mtr_packed_words(int32_t len) { return (int64_t)(len / 16) + 4; }
static inline mtr_status mtr_pack_read(const uint8_t *codes, int32_t len, uint32_t *dst_words)
{
    if (!codes || !dst_words || len <= 0) return MTR_ERR_BAD_ARG;
    const int32_t full = len >> 4;
    uint32_t seen = 0;
    for (int32_t q = 0; q < full; q++) {
        const uint8_t *c = codes + ((int64_t)q << 4);
        uint32_t v = 0, o = 0;
        for (int t = 0; t < 16; t++) { v = (v << 2) | c[t]; o |= c[t]; }
        dst_words[q] = v; seen |= o;
    }
    uint32_t v = 0;
    for (int32_t p = full << 4; p < len; p++) { v |= (uint32_t)codes[p] << (30 - 2 * (p & 15)); seen |= codes[p]; }
    dst_words[full] = v; dst_words[full + 1] = 0; dst_words[full + 2] = 0; dst_words[full + 3] = 0;
    return seen > 3 ? MTR_ERR_BAD_ARG : MTR_OK;
}
mtr_status mtr_upload_batch_packed(mtr_ctx *ctx, const uint32_t *packed, int64_t n_words, const int64_t *woff,
                                   const int32_t *lens, int32_t n_reads);

/* ---- reads already in device memory -------------------------------------------------------------------------------
 * mtr_upload_batch_device takes the reads as text in DEVICE memory on the context's GPU (a basecaller's output, a torch
 * tensor) and packs them on the device, by a kernel, into exactly the image mtr_upload_batch builds on the host.
 *   d_text       text_bytes bytes of device memory on the context's device, one byte per base:
 *                MTR_TEXT_ASCII 'A','C','G','T' or 'a','c','g','t'; MTR_TEXT_CODES 0..3 = A C G T (what mtr_upload_batch takes)
 *   offsets      n_reads HOST int64 start offsets into d_text;  lens  n_reads HOST lengths (1..MTR_MAX_READ_LENGTH)
 *   wait_stream  the hipStream_t the caller wrote d_text on (NULL = the null stream): the library records an event there and
 *                its own stream waits for that event (no device-wide synchronisation)
 * Returns after the packing has finished: d_text may then be reused.  Bytes of d_text outside every read are never looked at;
 * a byte inside a read that is not a base of the kind (e.g. 'N', '
', a code > 3) is MTR_ERR_BAD_ARG, and mtr_last_error names
 * the first such read.  So are d_text that is not device memory of the context's GPU, a read outside text_bytes, an unknown
 * text_kind.  A refused upload leaves no batch uploaded, as a refused mtr_upload_batch does; run / fetch / export / alignments
 * work after a device upload as after a host one.  File-order mode for reads in device memory: mtr_upload_batch_device_in_file
 * (below, with mtr_file_state). */
#define MTR_TEXT_ASCII 0
#define MTR_TEXT_CODES 1
mtr_status mtr_upload_batch_device(mtr_ctx *ctx, const uint8_t *d_text, int64_t text_bytes, const int64_t *offsets,
                                   const int32_t *lens, int32_t n_reads, int32_t text_kind, void *wait_stream);

/* ---- a FASTA file in device memory ---------------------------------------------------------------------------------------
 * The step in front of mtr_upload_batch_device: the bytes of a FASTA file in DEVICE memory on the context's GPU (read there
 * directly, or copied raw) are parsed by device kernels with the rules of the reference's reader (handle_one_file.c:169-269,
 * restated in mtr_amd/host/fasta.c and in mtr_amd/csrc/fasta.hip.inc): fgets windows of 4095 characters, a window that begins
 * with '>' is a header whose ID runs to the first NUL, LF or CR, such a character hides the rest of a sequence window, bases in
 * front of the first header join the first record.  The input stops at the first of: a character that is none of ACGTacgt
 * (MTR_FASTA_END_BADCHAR), a header that closes a record without bases (MTR_FASTA_END_EMPTY), a record's MTR_MAX_INPUT_LENGTH-th
 * base (MTR_FASTA_END_TOOLONG); the reads are the records closed before it.  Without such a stop the end of the file closes the
 * last record: MTR_FASTA_END_EOF, or MTR_FASTA_END_EMPTY if that record has no bases.  The values mean what MTRH_END_* of
 * mtr_amd/host/mtr_host.h mean.
 *   info      n_reads reads of n_bases bases in all, their IDs id_bytes bytes; end = why the input ended, end_pos = the position of
 *             the stop in d_fasta (n_bytes when the file ended), bad_char = the character of MTR_FASTA_END_BADCHAR
 *   dst       caller-owned DEVICE memory: text = the reads' bases, read after read, the file's own bytes (what
 *             mtr_upload_batch_device takes as MTR_TEXT_ASCII); read i = text[offsets[i] .. offsets[i] + lens[i]); its ID =
 *             ids[id_off[i] .. id_off[i + 1]), what the header holds behind '>'; id_off has n_reads + 1 entries
 * mtr_parse_fasta_device follows mtr_report_device's protocol: dst == NULL: MTR_OK with info only; a capacity below info's:
 * MTR_ERR_OVERFLOW with info filled, nothing written; else the columns are written and the context's stream synchronised before
 * the call returns.  A stop is no error: the status is MTR_OK and info->end tells.  n_bytes == 0: MTR_OK, no reads,
 * MTR_FASTA_END_EMPTY.  wait_stream as in mtr_upload_batch_device.  d_fasta that is NULL, not device memory of the context's GPU or
 * runs past its allocation, and n_bytes < 0 or > INT32_MAX are MTR_ERR_BAD_ARG.  The resident batch is not touched.
 * mtr_upload_fasta_device parses into buffers of the context and makes the reads the resident batch as mtr_upload_batch_device
 * does.  A stop does not refuse the upload: the reads before it are uploaded, as the command line prints the reads before a bad
 * record.  No reads: MTR_OK and no batch uploaded.  A read longer than MTR_MAX_READ_LENGTH: MTR_ERR_BAD_ARG naming the read, no
 * batch uploaded.  run / fetch / export / alignments / report work afterwards as after any upload.  File-order mode for a file in device
 * memory: mtr_upload_fasta_device_in_file (below, with mtr_file_state).
 * mtr_fasta_index: HOST copies of the last mtr_upload_fasta_device's index - lens[n_reads], id_off[n_reads + 1], ids[id_bytes] (what
 * mtr_report_text_device takes); a NULL array is skipped.  MTR_ERR_BAD_ARG before any such upload. */
#define MTR_FASTA_END_EOF 0
#define MTR_FASTA_END_EMPTY 1
#define MTR_FASTA_END_BADCHAR 2
#define MTR_FASTA_END_TOOLONG 3
typedef struct mtr_fasta_info { int32_t n_reads, end, bad_char, reserved; int64_t end_pos, n_bases, id_bytes; } mtr_fasta_info;
typedef struct mtr_fasta_dst {
    uint8_t *text;        /* [n_bases]                                        */
    int64_t *offsets;     /* [n_reads]                                        */
    int32_t *lens;        /* [n_reads]                                        */
    uint8_t *ids;         /* [id_bytes]                                       */
    int64_t *id_off;      /* [n_reads + 1]                                    */
    int64_t  cap_text, cap_reads, cap_id_bytes;
} mtr_fasta_dst;
mtr_status mtr_parse_fasta_device(mtr_ctx *ctx, const uint8_t *d_fasta, int64_t n_bytes, void *wait_stream,
                                  const mtr_fasta_dst *dst, mtr_fasta_info *info);
mtr_status mtr_upload_fasta_device(mtr_ctx *ctx, const uint8_t *d_fasta, int64_t n_bytes, void *wait_stream, mtr_fasta_info *info);
mtr_status mtr_fasta_index(const mtr_ctx *ctx, int32_t *lens, int64_t *id_off, char *ids);

/* ---- a FASTQ file in device memory ---------------------------------------------------------------------------------------
 * What the long-read basecallers write, parsed by device kernels (mtr_amd/csrc/fastq.hip.inc).  The reference has no FASTQ reader;
 * the rules are this library's: strict four-line FASTQ.
 *   lines      line 0 starts at byte 0; line l + 1 starts behind the l-th LF, if a byte exists there (no fgets windows)
 *   content    a line's content is its bytes in front of its first NUL, LF or CR, the FASTA rules' terminators; a terminator
 *              hides the rest of its line
 *   record r   is lines 4r .. 4r + 3 - header: content begins with '@', the ID is the content behind it, spaces included, and may
 *              be empty; sequence: every content byte is one of ACGTacgt; separator: content begins with '+', the rest is
 *              ignored; quality: content as long as the sequence's content, its bytes are not looked at otherwise ('@', '>' and
 *              '+' are legal first quality characters and are not taken for a header)
 *   stop       the input stops at the first of these in file order:
 *                MTR_FASTA_END_BADCHAR  a sequence content byte outside ACGTacgt, 'N' included: end_pos at that byte, bad_char
 *                                       holds it
 *                MTR_FASTA_END_TOOLONG  the MTR_MAX_INPUT_LENGTH-th base of a sequence line: end_pos at that base
 *                MTR_FASTA_END_EMPTY    a sequence line with empty content: end_pos = the line's first byte
 *                MTR_FASTA_END_FORMAT   a header line not beginning with '@' or a separator line not beginning with '+': end_pos =
 *                                       the line's first byte; a quality line whose content length differs from the sequence's:
 *                                       end_pos = the line's first byte; the file ends inside a record, so fewer than four lines
 *                                       of it begin: end_pos = n_bytes.  A blank line behind the last record is a header line
 *                                       without '@'
 *   reads      the records whose four lines are complete and correct before the stop; a last quality line without LF is complete
 *   no stop    MTR_FASTA_END_EOF.  n_bytes == 0: MTR_OK, no reads, MTR_FASTA_END_EMPTY, as for FASTA
 * Protocol, argument checks and stream handling are those of the FASTA entry points above, and info, dst, mtr_fasta_index mean
 * what they mean there: text = the reads' bases read after read, offsets their exclusive sum.  mtr_upload_fastq_device compacts
 * nothing: a sequence line is contiguous in the file, and the packing kernel of mtr_upload_batch_device reads the reads out of
 * d_fastq itself.  Multi-line FASTQ is not supported.  The qualities are no output of these calls; an upload keeps them with the
 * batch when mtr_keep_qualities is on ("qualities of the resident batch", below). */
#define MTR_FASTA_END_FORMAT 4
mtr_status mtr_parse_fastq_device(mtr_ctx *ctx, const uint8_t *d_fastq, int64_t n_bytes, void *wait_stream,
                                  const mtr_fasta_dst *dst, mtr_fasta_info *info);
mtr_status mtr_upload_fastq_device(mtr_ctx *ctx, const uint8_t *d_fastq, int64_t n_bytes, void *wait_stream, mtr_fasta_info *info);

/* ---- wire form of the record table -------------------------------------------------------------------------------
 * A mtr_record is 2560 bytes because unit[] and unit_score[] are sized for MAX_PERIOD; a typical record uses 600.  The
 * wire form keeps what insert_an_alignment_into_set receives and nothing else, record after record:
 *   14 int32 (rep_start .. reserved, as in mtr_record) | rep_period unit bytes 'A','C','G','T', zero-padded to a
 *   multiple of 4 | rep_period int32 unit scores.
 * mtr_fetch_results_packed: the records of the last run in wire form, compacted on the device and copied into PINNED
 * host memory owned by the context (valid until the next upload / fetch on this context; do not free).  Reads
 * first_read .. first_read+n-1 only when n_reads_limit >= 0 (after MTR_ERR_DP_TOO_LARGE: the reads before the failing
 * one); pass -1 for all.  mtr_export_packed_device: the same into caller-owned DEVICE memory (for RCCL).
 * mtr_unpack_records / mtr_pack_records convert on the host (no device needed). */
#define MTR_WIRE_HEADER_BYTES 56
static inline int64_t mtr_wire_record_bytes(int32_t rep_period)
{
    const int64_t p = rep_period < 0 ? 0 : (rep_period > MTR_MAX_PERIOD ? MTR_MAX_PERIOD : rep_period);
    return MTR_WIRE_HEADER_BYTES + ((p + 3) & ~(int64_t)3) + 4 * p;
}
mtr_status mtr_fetch_results_packed(mtr_ctx *ctx, int32_t n_reads_limit, const uint8_t **out_blob, int64_t *out_bytes,
                                    const int32_t **out_counts, int64_t *out_total_records);
mtr_status mtr_export_packed_device(mtr_ctx *ctx, void *d_dst, int64_t capacity_bytes, int32_t *counts_host,
                                    int64_t *out_total_records, int64_t *out_bytes);
/* out must hold n_records entries; only the fields a record carries are written (unit is NUL-terminated) */
mtr_status mtr_unpack_records(const uint8_t *blob, int64_t bytes, int64_t n_records, mtr_record *out);
/* returns the number of bytes written, or -1 if capacity is too small */
int64_t    mtr_pack_records(const mtr_record *records, int64_t n_records, uint8_t *out, int64_t capacity);

/* ---- mTR's report on the device ------------------------------------------------------------------------------------------
 * mTR's report on the device: per read the maximum-score chain of its records (chaining.cpp:243-363, ties in insertion order,
 * exactly mtr_amd/host/chain.c), reads in input order, each read's repeats in print order.  The columns are caller-owned DEVICE
 * memory on the context's GPU. */
typedef struct mtr_report_dst {
    int32_t *read;        /* [R]    read index                                                               */
    int32_t *record;      /* [R]    index of the repeat among its read's records (insertion order, as fetch) */
    int32_t *fields;      /* [R*14] the 14 header ints of mtr_record (0-origin positions)                    */
    float   *ratio;       /* [R]    (float)num_matches / repeat_len - the printed "match ratio"              */
    int64_t *unit_off;    /* [R+1]  units[unit_off[k] .. unit_off[k+1]) = repeat k's unit, ASCII             */
    uint8_t *units;       /* [U]                                                                             */
    int64_t  cap_repeats, cap_unit_bytes;
} mtr_report_dst;
/* As mtr_export_packed_device: the chains are made on the first call after a run (and kept until the next upload or run);
 * counts_host[i] = repeats of read i, *out_repeats = R, *out_unit_bytes = U.  dst == NULL: MTR_OK with the sizes only; capacities
 * below R / U: MTR_ERR_OVERFLOW with the sizes; else the columns are written and the context's stream synchronised before the
 * call returns.  Before any run MTR_ERR_BAD_ARG; after a failed run the status that run latched. */
mtr_status mtr_report_device(mtr_ctx *ctx, const mtr_report_dst *dst, int32_t *counts_host, int64_t *out_repeats, int64_t *out_unit_bytes);

/* ---- the -a alignments of the report's repeats, on the device ------------------------------------------------------------------
 * The alignment between the read and the predicted tandem repeat (the reference's -a: wrap_around_DP.c:57-213, chaining.cpp:164-167)
 * of every repeat of mtr_report_device, in its order: repeat k here is repeat k there, R the same.  The reads' 2-bit image, the
 * records and the chains are resident after a run, so no base, unit, record or path byte crosses to the host: device kernels make the
 * tasks, mtr_alignments' kernel aligns them, and a kernel renders each path into caller-owned DEVICE memory on the context's GPU -
 * in FORWARD (print) order, the order in which print.c's alignment_block prints the columns, 50 to a block.
 *   column c of repeat k (col_off[k] <= c < col_off[k+1]):  ops[c] = 1 match, 2 mismatch, 3 gap in the read, 4 gap in the unit;
 *   text[c] = the read's base or '-', text[C + c] = '|' for a match, else ' ', text[2C + c] = the unit's base or '-'   (C = *out_columns);
 *   first[2k] = 0-origin read position, first[2k+1] = 1-origin unit column at repeat k's FIRST column (0, 0 for a repeat without columns).
 * A repeat with rep_period <= 0 or an empty path has zero columns (alignment_block prints only its scores line).  A read position one
 * or two past the read's end shows what mtr_get_bases_after_read reports ('A' under isolated semantics).
 * Protocol as mtr_report_device: the alignments are made on the first call after a run (which makes the chains too if mtr_report_device
 * has not been called) and kept until the next upload or run; *out_repeats = R, *out_columns = C.  dst == NULL: MTR_OK with the sizes
 * only; capacities below R / C: MTR_ERR_OVERFLOW with the sizes, nothing written; else the columns are written and the context's stream
 * synchronised before the call returns.  Before any run MTR_ERR_BAD_ARG; after a failed run the status that run latched. */
typedef struct mtr_report_align_dst {
    int64_t *col_off;     /* [R+1]  columns of repeat k = col_off[k] .. col_off[k+1]                              */
    uint8_t *ops;         /* [C]                                                                                  */
    uint8_t *text;        /* [3*C]  row r at text + r*C                                                           */
    int32_t *first;       /* [R*2]                                                                                */
    int64_t  cap_repeats, cap_columns;
} mtr_report_align_dst;
mtr_status mtr_report_alignments_device(mtr_ctx *ctx, const mtr_report_align_dst *dst, int64_t *out_repeats, int64_t *out_columns);

/* ---- the report as text, on the device ---------------------------------------------------------------------------------------------
 * The bytes mTR writes to stdout for the resident batch, formatted by device kernels into caller-owned DEVICE memory on the context's
 * GPU: per repeat of mtr_report_device the line of mtr_amd/host/print.c's report_line (ID, L, start+1, end+1, repeat_len, period,
 * copies, matches, the ratio as printf("%f") of (float)num_matches / repeat_len, mismatches, insertions, deletions, unit; tabs between,
 * a line feed behind) and, with_alignments != 0, the block of alignment_block behind it (mTR -a: an empty line, the scores line, an
 * empty line, then per 50 columns of the repeat's alignment its three rows and an empty line).  No byte of a record, unit or path
 * crosses to the host.  The ratio's float is the ratio column of mtr_report_device bit for bit; 0 / 0 prints "-nan", as print.c on an
 * x86 host (no record the library makes has repeat_len 0).
 * ids / id_off are HOST arrays, the only caller data the report needs that the context does not have: read i's ID is the bytes
 * ids[id_off[i] .. id_off[i+1]) - what the FASTA header holds behind '>' -, written verbatim; id_off has n_reads + 1 non-decreasing
 * entries.  They are copied to the device per call and free again when it returns.
 * Protocol as mtr_report_device: the chains, and for with_alignments the alignments, are made on first use after a run and kept until
 * the next upload or run, so this call, mtr_report_device and mtr_report_alignments_device may come in any order and any mix, and both
 * modes one after the other.  *out_bytes = B.  dst == NULL: MTR_OK with B only; cap_bytes below B: MTR_ERR_OVERFLOW with B, nothing
 * written; else text and read_off are written and the context's stream synchronised before the call returns.  Before any run
 * MTR_ERR_BAD_ARG; after a failed run the status that run latched; NULL ids / id_off or a decreasing id_off MTR_ERR_BAD_ARG. */
typedef struct mtr_report_text_dst {
    uint8_t *text;        /* [B]  mTR's stdout for the resident batch: reads in input order, each read's repeats in print order */
    int64_t *read_off;    /* [n_reads+1] or NULL: read i's bytes are text[read_off[i] .. read_off[i+1]) */
    int64_t  cap_bytes;
} mtr_report_text_dst;
mtr_status mtr_report_text_device(mtr_ctx *ctx, const char *ids, const int64_t *id_off, int32_t with_alignments,
                                  const mtr_report_text_dst *dst, int64_t *out_bytes);

/* ---- the motif catalogue of the report's repeats, on the device -------------------------------------------------------------------------
 * "Which repeats are the same repeat?"  mTR prints a unit in whatever phase and strand the read had: CAG, AGC, GCA and CTG (the other
 * strand) are one motif.  For every repeat of mtr_report_device, in its order (repeat k here is repeat k there, R the same), device kernels
 * find the canonical motif and the strand and rotation that lead to it, and group the repeats of the resident batch by motif; no unit
 * crosses to the host.  The reference has no such output; this is its definition:
 *   unit u      what mtr_report_device writes for the repeat: strnlen(unit, rep_period) bytes over ACGT, 0 <= p <= 500 of them
 *   rc(u)       the reverse complement;  rot(s, r)[i] = s[(i + r) mod p];  strings compare bytewise, so A < C < G < T
 *   canon(u)    the smallest string among the 2p strings rot(u, r) and rot(rc(u), r);  strand = 0 if some rot(u, r) attains it (the forward
 *               strand wins a tie), else 1;  rotation = the smallest r on that strand that attains it
 *   motif_len   d = the smallest divisor of p with rot(canon, d) == canon;  the motif is canon[0 .. d): ACAC, CA and GT all have motif AC
 *               (and rotation < d always);  p == 0: strand = rotation = motif_len = 0 and the empty motif
 *   group       two repeats are in one group iff their motifs are equal as strings (compared byte for byte, never by hash alone); groups are
 *               numbered 0 .. G-1 by the report index of their first repeat
 *   per group   g_first = that first repeat's k;  g_repeats = its members;  g_reads = the distinct reads with a member;  g_copies = the sum
 *               over the members of num_freq_unit * (p / d) (0 for a member with p == 0);  g_bases = the sum of their repeat_len
 * The sums are integer sums: the catalogue of a batch does not depend on how the device scheduled the work.
 * The columns are caller-owned DEVICE memory on the context's GPU.  Protocol as mtr_report_device: the catalogue is made on first use after
 * a run (which makes the chains too if nobody has asked for them yet) and kept until the next upload or run, so this call and the three
 * other report calls may come in any order and any mix; *out_repeats = R, *out_groups = G, *out_motif_bytes = M.  dst == NULL: MTR_OK with
 * the sizes only; a capacity below its size: MTR_ERR_OVERFLOW with the sizes, nothing written; a NULL column that would be written:
 * MTR_ERR_BAD_ARG (motif_off is always written: motif_off[G] = M, also for R == 0); else the columns are written and the context's stream
 * synchronised before the call returns.  Before any run MTR_ERR_BAD_ARG; after a failed run the status that run latched. */
typedef struct mtr_report_motif_dst {
    uint8_t *strand;  int32_t *rotation, *motif_len, *group;                 /* [R] */
    int64_t *motif_off;  uint8_t *motifs;                                    /* [G+1], [M]: group g's motif = motifs[motif_off[g] .. motif_off[g+1]) */
    int32_t *g_first, *g_repeats, *g_reads;  int64_t *g_copies, *g_bases;    /* [G] */
    int64_t  cap_repeats, cap_groups, cap_motif_bytes;
} mtr_report_motif_dst;
mtr_status mtr_report_motifs_device(mtr_ctx *ctx, const mtr_report_motif_dst *dst,
                                    int64_t *out_repeats, int64_t *out_groups, int64_t *out_motif_bytes);

/* ---- known-motif search: given motifs aligned to every read, on the device ----------------------------------------------------------------
 * "I know the motif (CAG, GGGGCC, a 33-base VNTR unit): where is it in every read, and with how many copies?"  The report answers for the units
 * the search infers; this call aligns the caller's motifs to every read of the resident batch by the wrap-around DP itself and returns one hit
 * per (read, motif).  It needs an uploaded batch and no run: it may come before or after one (a run in flight ends first), it reads the reads
 * alone - no after-base, so file-order mode does not change a hit - and the records, chains, kept reports and motif catalogue of the batch stay
 * as they are.  This is its definition, in clean coordinates:
 *   read x[0 .. L), motif m[0 .. U) over ACGT with 1 <= U <= 499, scores G (gain), MM (mismatch), D (indel)
 *   a hit       the result of the reference's wrap_around_DP_sub (wrap_around_DP.c:222-354) with DP row i (1 .. L) standing for read base x[i - 1]:
 *               every base of the read is aligned and nothing past its end is read (the reference's own callers read org[query_start + i]; this
 *               entry does not copy that off-by-one)
 *   recurrence  (:258-285) H(0, j) = 0;  a match gives H(i, j) = H(i-1, j-1) + G;  otherwise H(i, j) = max(0, H(i-1, j-1) - MM, H(i-1, j) - D,
 *               H(i, j-1) - D), without the last term in column 1;  the wrap is H(i, 0) = H(i, U)
 *   best cell   the first strict maximum in row-major order (max_i, max_j)
 *   traceback   (:298-333) from the best cell while i > 0 and H > 0, in the fixed priority order match, mismatch, deletion (j - 1, from column 1 to
 *               column U of the same row), insertion (i - 1)
 *   columns     start = 0-origin index of the first aligned base = the traceback's final i;  end = 0-origin, inclusive = max_i - 1;
 *               repeat_len = end - start + 1;  copies = (matches + mismatches + deletions) / U;  matches, mismatches, insertions, deletions;
 *               score = the best cell's value (= G * matches - MM * mismatches - D * (insertions + deletions));
 *               ratio = (float)matches / repeat_len, 0 when repeat_len == 0
 *   no hit      a read with no positive cell: start = 0, end = -1 and zeros everywhere else
 *   strands     both_strands != 0: the reverse complement of the motif is aligned as well, the hit is the alignment with the higher score, the forward
 *               motif wins a tie; strand = 0 or 1 says which won (a palindromic motif such as AT is always strand 0).  both_strands == 0: strand = 0
 *   as given    the motif is not reduced to a primitive period and not rotated: ACAC counts copies of four bases
 * This equals the oracle's wrap_around_DP_sub on the read shifted by one base (window 0 .. L - 1 of [any base] + x) with rep_start and rep_end each
 * lowered by one.
 * motifs / motif_off are HOST arrays, as ids / id_off of mtr_report_text_device: motif k is motifs[motif_off[k] .. motif_off[k + 1]), upper-case ACGT.
 * The columns are caller-owned DEVICE memory on the context's GPU; hit h = read * n_motifs + motif, H = n_reads * n_motifs of them.
 * Checked in this order: MTR_ERR_BAD_ARG (mtr_last_error names the offender) without an uploaded batch, for n_motifs <= 0, gain outside 1..5, mismatch
 * or indel outside 1..3 (the ranges the forward passes are written and tested for), a decreasing motif_off, a motif of length 0 or over 499, a byte
 * outside ACGT, more than 2^30 - 1 motifs or motif bases, H over 2^31 - 1;  MTR_ERR_DP_TOO_LARGE, decided on the host before any launch, if for any (read, motif) (U + 1) * L + U reaches the
 * WrapDPsize the kernels use (the message names the read and the motif);  then *out_hits = H and, as the report calls: dst == NULL: MTR_OK with the
 * size only;  cap_hits < H: MTR_ERR_OVERFLOW, nothing written;  a NULL column: MTR_ERR_BAD_ARG;  else the columns are written and the context's
 * stream synchronised before the call returns. */
typedef struct mtr_motif_hits_dst {
    int32_t *fields;   /* [H*8] start, end, repeat_len, copies, matches, mismatches, insertions, deletions */
    int32_t *score;    /* [H] */
    float   *ratio;    /* [H] */
    uint8_t *strand;   /* [H] */
    int64_t  cap_hits;
} mtr_motif_hits_dst;   /* caller-owned DEVICE memory; hit h = read * n_motifs + motif */
mtr_status mtr_search_motifs_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, int32_t n_motifs,
                                    int32_t gain, int32_t mismatch, int32_t indel, int32_t both_strands,
                                    const mtr_motif_hits_dst *dst, int64_t *out_hits);

/* ---- known-motif search: every locus of a motif in a read, not only the best -----------------------------------------------------------------
 * mtr_search_motifs_device answers with ONE hit per (read, motif), the best local alignment; a long read or a contig holds a motif at several
 * places.  This call reports all of them that reach a score, by aligning what lies left and right of a hit again.  The definition, for a read
 * x[0 .. L), a motif m, the scores G, MM, D and both_strands of the search, a threshold min_score = S >= 1 and max_rounds = R in 1..32, with
 * minlen = ceil(S / G) (a locus of score S holds at least that many read bases):
 *   loci(lo, hi, depth):                          the half-open window x[lo .. hi)
 *       if hi - lo < minlen: return
 *       if depth == R: open = 1; return           the pair's "open" flag: something may be left
 *       (hit, strand) = the hit of mtr_search_motifs_device's definition above, verbatim, for the read x[lo .. hi): both strands, the higher
 *                       score wins, the forward motif on a tie
 *       if hit.score < S: return
 *       emit the hit with start and end raised by lo, and its strand
 *       loci(lo, lo + hit.start, depth + 1);  loci(lo + hit.end + 1, hi, depth + 1)
 *   the loci of (read, motif) = loci(0, L, 0), reported in ascending start
 * A reported hit has repeat_len >= 1, so both children are strictly shorter and the recursion ends; the loci of a pair never overlap; with R = 1
 * the result is mtr_search_motifs_device's hit where its score reaches S and nothing otherwise; skipping a window shorter than minlen never
 * changes a result.
 * The number of loci T is known only after the work, so there are two entry points: the search keeps its result in buffers of the context, the
 * copy hands it out.
 * mtr_search_motif_loci_device: the protocol of mtr_search_motifs_device - a run in flight ends first, an uploaded batch is needed and no run is,
 * nothing a run left is touched, its own status word and counters.  The checks are the search's in the search's order, with MTR_ERR_BAD_ARG for
 * min_score < 1 and for max_rounds outside 1..32 after the other arguments' and before MTR_ERR_DP_TOO_LARGE, which is decided from the whole reads
 * before any launch, as there.  MTR_ERR_OVERFLOW if one round holds more than 2^31 - 1 alignments or the loci exceed 2^31 - 1.  On MTR_OK
 * *out_pairs = P = n_reads * n_motifs, *out_loci = T and the result is kept; a failed call keeps nothing.  An upload of any kind and the next locus
 * search (whatever its outcome) discard what is kept; a run does not.
 * mtr_motif_loci_copy_device copies the kept result, device to device, into caller-owned DEVICE memory of the context's GPU:
 *   loci_off   [P + 1]   the loci of pair p = read * n_motifs + motif are rows loci_off[p] .. loci_off[p + 1], in ascending start
 *   fields     [T * 8]   the search's eight columns, in read coordinates;  score [T];  ratio [T], the search's formula;  strand [T]
 *   open       [P]       1: the recursion reached depth R on a window of at least minlen bases - a larger max_rounds may find more
 * MTR_ERR_BAD_ARG if nothing is kept or dst is NULL; MTR_ERR_OVERFLOW if cap_pairs < P or cap_loci < T, and then nothing is written;
 * MTR_ERR_BAD_ARG if loci_off or open is NULL, or with T > 0 any other column; else the columns are written and the context's stream is
 * synchronised before the call returns.  Two searches with the same arguments give byte-identical columns. */
typedef struct mtr_motif_loci_dst {
    int64_t *loci_off; /* [P+1] */
    int32_t *fields;   /* [T*8] start, end, repeat_len, copies, matches, mismatches, insertions, deletions */
    int32_t *score;    /* [T] */
    float   *ratio;    /* [T] */
    uint8_t *strand;   /* [T] */
    uint8_t *open;     /* [P] */
    int64_t  cap_pairs, cap_loci;
} mtr_motif_loci_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_search_motif_loci_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, int32_t n_motifs,
                                        int32_t gain, int32_t mismatch, int32_t indel, int32_t both_strands,
                                        int32_t min_score, int32_t max_rounds, int64_t *out_pairs, int64_t *out_loci);
mtr_status mtr_motif_loci_copy_device(mtr_ctx *ctx, const mtr_motif_loci_dst *dst);

/* ---- flank search: short patterns matched approximately against every read --------------------------------------------------------------------
 * Reads carry no coordinates: a locus is named by the unique sequence either side of its repeat.  This call matches every given pattern (a flank,
 * a primer, an adapter) approximately against every read of the resident batch and reports where it fits best.  The reference has nothing of this
 * kind; the definition is this project's own.  For a read x[0 .. L) and a pattern p[0 .. m) over ACGT, 1 <= m <= 64, with the unit-cost edit
 * distance ed (substitution, insertion and deletion cost 1 each):
 *   d(e)     = min over 0 <= s <= e of ed(p, x[s .. e)), for e = 0 .. L; d(0) = m
 *   dist     = min over e of d(e)
 *   end      = the smallest e with d(e) = dist
 *   start    = the largest s <= end with ed(p, x[s .. end)) = dist: the shortest such substring; end - start <= m + dist
 *   strands  both_strands != 0: the reverse complement of p is searched as well, the smaller dist wins, the forward pattern wins a tie; strand = 0
 *            or 1 says which won (a palindromic pattern is always strand 0).  both_strands == 0: strand = 0
 *   always   a hit is reported for every (read, pattern), without a threshold: the pattern matches x[start .. end) - half-open, end exclusive -
 *            with dist edits.  A read shorter than the pattern simply has a large dist; dist = m means start = end = 0 (nothing of the read
 *            helps)
 * The protocol is mtr_search_motifs_device's: an uploaded batch is needed and a run is not, a run in flight ends first, nothing kept of the batch
 * is touched (the call has its own status word and counters), patterns / pattern_off are HOST arrays as motifs / motif_off, the columns are
 * caller-owned DEVICE memory on the context's GPU, hit h = read * n_patterns + pattern, H = n_reads * n_patterns of them.
 * Checked in this order: MTR_ERR_BAD_ARG (mtr_last_error names the offender) without an uploaded batch, for n_patterns <= 0, a decreasing
 * pattern_off, a pattern of length 0 or over 64, a byte outside ACGT, H over 2^31 - 1;  then *out_hits = H and, as the report calls: dst == NULL:
 * MTR_OK with the size only;  cap_hits < H: MTR_ERR_OVERFLOW, nothing written;  a NULL column: MTR_ERR_BAD_ARG;  else the columns are written and
 * the context's stream synchronised before the call returns. */
typedef struct mtr_flank_hits_dst {
    int32_t *dist;     /* [H] */
    int32_t *start;    /* [H] 0-origin */
    int32_t *end;      /* [H] 0-origin, exclusive */
    uint8_t *strand;   /* [H] */
    int64_t  cap_hits;
} mtr_flank_hits_dst;   /* caller-owned DEVICE memory; hit h = read * n_patterns + pattern */
mtr_status mtr_search_flanks_device(mtr_ctx *ctx, const char *patterns, const int64_t *pattern_off, int32_t n_patterns,
                                    int32_t both_strands, const mtr_flank_hits_dst *dst, int64_t *out_hits);

/* ---- locus genotyping: the repeat between two flanks, counted -------------------------------------------------------------------------------------
 * "How many copies does this read carry at this locus?"  The motif alone does not identify a locus (a read holds CAG tracts at several places), and
 * a local alignment's ends do not delimit the allele (they are where the score happened to peak: an interrupted allele is cut short, an allele of 0
 * or 1 copies is invisible).  A locus is (A, M, B): left flank, motif, right flank; flanks of 1..64 bases, a motif as the search's, 1..499 bases.
 * The definition, for a read x, a locus (A, M, B), K = max_flank_dist >= 0, the scores G, MM, D of the search, rc = reverse complement, and F(p) =
 * the flank search's hit of pattern p on ONE strand (both_strands = 0, above):
 *   orientation 0   a = F(A), b = F(B); valid iff a.dist <= K, b.dist <= K and a.end <= b.start; the window is [a.end, b.start), the motif is M
 *   orientation 1   a' = F(rc A), b' = F(rc B); valid iff a'.dist <= K, b'.dist <= K and b'.end <= a'.start; the window is [b'.end, a'.start), the
 *                   motif is rc M
 *   choice          the read spans the locus in the valid orientation; if both are valid, the one with the smaller sum of its two distances,
 *                   orientation 0 on a tie; if neither is valid: spanning = 0 and every other column of the row is 0
 *   flank_dist      (left, right) = (a.dist, b.dist), or (a'.dist, b'.dist): each named by the locus' flank, not by its place in the read
 *   alignment       window [lo, hi) with lo < hi: the hit of mtr_search_motifs_device's definition, verbatim, for the read x[lo .. hi) against the
 *                   orientation's motif as given (both_strands = 0), with start and end raised by lo (a window without a positive cell: start = lo,
 *                   end = lo - 1, zeros elsewhere);  lo == hi, an allele of no copies: spanning = 1, eight zero fields, score 0, ratio 0, and no DP
 * The allele is hi - lo bases and fields[3] copies.
 * seqs / seq_off are HOST arrays as motifs / motif_off holding 3 * n_loci sequences: locus l is sequences 3l (left flank), 3l + 1 (motif), 3l + 2
 * (right flank).  The columns are caller-owned DEVICE memory, row = read * n_loci + locus.  The protocol is the flank search's; the call keeps
 * nothing and drops nothing the batch keeps.
 * Checked in this order: MTR_ERR_BAD_ARG without an uploaded batch, for n_loci <= 0, a decreasing seq_off;  the search's checks of the scores and
 * of the motifs (the message's "motif l" is locus l);  a flank of length 0 or over 64 or with a byte outside ACGT;  max_flank_dist < 0;  more than
 * 2^30 - 1 rows;  MTR_ERR_DP_TOO_LARGE, decided on the host from the WHOLE reads as the search decides it;  then *out_rows = n_reads * n_loci and
 * dst as above (cap_rows). */
typedef struct mtr_genotypes_dst {
    uint8_t *spanning;     /* [R] */
    uint8_t *orientation;  /* [R] */
    int32_t *flank_dist;   /* [R*2] left, right */
    int32_t *window;       /* [R*2] lo, hi */
    int32_t *fields;       /* [R*8] start, end, repeat_len, copies, matches, mismatches, insertions, deletions: read coordinates */
    int32_t *score;        /* [R] */
    float   *ratio;        /* [R] */
    int64_t  cap_rows;
} mtr_genotypes_dst;   /* caller-owned DEVICE memory; row = read * n_loci + locus */
mtr_status mtr_genotype_loci_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist,
                                    int32_t gain, int32_t mismatch, int32_t indel, const mtr_genotypes_dst *dst, int64_t *out_rows);

/* ---- catalogue genotype: the genotype's spanning rows for a locus list of any length ---------------------------------------------------------------
 * mtr_genotype_loci_device scans every read against every flank and writes a row per (read, locus): a catalogue of tens of thousands of loci, of
 * which a read spans a handful, does not fit it.  This call returns exactly the rows that call would write with spanning = 1 - every column bit for
 * bit - as a list sorted by (read, locus), and does no work sized reads x loci.  It is not an approximation:
 *   seeds       a pattern p of m bases, K = max_flank_dist and q = seed_len with m >= (K + 1) * q has the K + 1 disjoint seeds p[i * q .. i * q + q),
 *               i = 0 .. K.  A substring of the read within K edits of p leaves at least one seed untouched: that seed occurs in the read exactly.
 *   candidate   (read, locus, orientation o) where the read holds a seed of BOTH patterns of o - A and B for o = 0, rc A and rc B for o = 1 (the
 *               seeds of the reverse complement are taken from the reverse complement).  Every other orientation is invalid by the genotype's
 *               definition, whatever its flank hits are.
 *   rows        for a candidate the two flank hits F(.) are the genotype's own; the pairing rule runs with a non-candidate orientation counted
 *               as invalid, and a spanning (read, locus) is a row: read, locus, and the seven columns as mtr_genotype_loci_device defines them.
 * The number of rows R is known only after the work, so there are two entry points, as the locus search's: the context keeps the result, the copy
 * hands it out.
 * mtr_genotype_catalog_device: seqs / seq_off, the scores and the protocol are mtr_genotype_loci_device's, and so are the checks, in its order,
 * including the limit of 2^30 - 1 (read, locus) pairs - the alignment path's pair ids are 32-bit (read * 2 * n_loci + 2 * locus + orientation), so a
 * catalogue is limited by n_reads * n_loci although nothing of that size is allocated - and MTR_ERR_DP_TOO_LARGE, decided from the whole reads.
 * Then MTR_ERR_BAD_ARG for seed_len outside 8..16 and for a flank shorter than (max_flank_dist + 1) * seed_len (mtr_last_error names the locus and
 * the side).  MTR_ERR_OVERFLOW for more than 2^31 - 1 seed hits or 2^30 - 1 candidates.  On MTR_OK *out_rows = R, *out_candidates = the number of
 * (read, locus, orientation) candidates verified (how selective the seeds were), and the rows are kept; a failed call keeps nothing.  An upload of
 * any kind and the next catalogue call (whatever its outcome) discard what is kept; a run, the locus search and the other genotype calls do not.
 * mtr_genotype_catalog_copy_device copies the kept rows, device to device, into caller-owned DEVICE memory of the context's GPU: read [R] and
 * locus [R], ascending by (read, locus), and rows.* with R rows (spanning is 1 throughout).  MTR_ERR_BAD_ARG if nothing is kept or dst is NULL;
 * MTR_ERR_OVERFLOW if rows.cap_rows < R, and then nothing is written; MTR_ERR_BAD_ARG if R > 0 and a column is NULL; else the columns are written
 * and the context's stream is synchronised before the call returns.  Two calls with the same arguments give byte-identical columns.
 * What the call is meant for: seeds that are rare in the reads.  A position's cost is one filter look; a seed hit costs a table probe and an entry
 * per (locus, slot) that has the seed, and a read's hits are compared pairwise to find its candidates (quadratic in the read's hits).  With
 * 4^seed_len well above the catalogue's 4 * (max_flank_dist + 1) * n_loci seeds - seed_len >= 12 for 100 000 loci - a 2 kb read has tens to
 * hundreds of hits; at seed_len = 8 (65 536 codes) a catalogue of more than a few thousand loci makes every position a hit of several entries
 * and the call slower than the dense one.  Choose the largest seed_len the flanks admit. */
typedef struct mtr_catalog_dst {
    int32_t *read;           /* [R] */
    int32_t *locus;          /* [R] */
    mtr_genotypes_dst rows;  /* the genotype's columns, R rows; cap_rows is the capacity of all nine */
} mtr_catalog_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_genotype_catalog_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist,
                                       int32_t seed_len, int32_t gain, int32_t mismatch, int32_t indel, int64_t *out_rows,
                                       int64_t *out_candidates);
mtr_status mtr_genotype_catalog_copy_device(mtr_ctx *ctx, const mtr_catalog_dst *dst);

/* ---- partial genotype: what a read that does not span a locus still proves ------------------------------------------------------------------------
 * The genotype answers only for reads that span a locus; an expanded allele is the one a read is least likely to span.  A read that holds one
 * flank and runs off its end inside the repeat proves "at least N copies"; a read whose repeat ends but whose far flank is too damaged to be found
 * carries a count as well.  This call reports both.  The reference has nothing of this kind; the definition is this project's own.  For a read
 * x[0 .. L), a locus (A, M, B) and K, G, MM, D as the genotype's, max_tail >= 0, and the four single-strand flank hits of the genotype's definition
 * as slots: 0 = F(A), 1 = F(B), 2 = F(rc A), 3 = F(rc B):
 *   partial row   iff the genotype's pairing rule finds neither orientation valid (it would say spanning = 0) and at least one slot has dist <= K.
 *                 A spanning row, and a row with no flank within K, is all zeros
 *   slot          the slot of smallest dist among those with dist <= K, the lowest slot number on a tie.  It fixes the window [lo, hi), the
 *                 direction and the motif Mo:
 *                   slot 0 (A)      [a.end, L)      forward from lo     M
 *                   slot 1 (B)      [0, b.start)    backward from hi    M
 *                   slot 2 (rc A)   [0, a'.start)   backward from hi    rc M
 *                   slot 3 (rc B)   [b'.end, L)     forward from lo     rc M
 *                 forward: y[t] = x[lo + t], m[j] = Mo[j];  backward: y[t] = x[hi - 1 - t], m[j] = Mo[U - 1 - j];  n = hi - lo
 *   extension     of y[0 .. n) against m[0 .. U), 1 <= U <= 32: the search's wrap-around recurrence ANCHORED at the flank, that is, without the
 *                 maximum with 0.  Row 0: H(0, j) = C(0, j) = T(0, j) = 0 for every j (the phase at the flank is free).  Rows i = 1 .. n, columns
 *                 j = 1 .. U, with H(i - 1, 0) = H(i - 1, U) (C and T likewise):
 *                   sub  = H(i - 1, j - 1) + (G if y[i - 1] == m[j - 1], else -MM)
 *                   left = H(i, j - 1) - D, for j > 1 only (column 1 has no left term, as in the search's forward pass)
 *                   up   = H(i - 1, j) - D
 *                 H(i, j) is the largest of these; the predecessor is the first of sub, left, up that attains it (the traceback's order:
 *                 diagonal, deletion, insertion).  C counts motif bases consumed: the predecessor's C, plus 1 for sub and for left.  T counts
 *                 matches: the predecessor's T, plus 1 for a matching sub.
 *   best cell     (bi, bj) = the first strict maximum of H in row-major order over the rows >= 1, if it is positive.  Without a positive cell, or
 *                 with n = 0: bi = 0 and C = T = H = 0
 *   columns       partial;  slot;  flank_dist = the slot's dist;  window = lo, hi;  ext = ext_len = bi, motif_bases = C(bi, bj), copies = C / U,
 *                 matches = T(bi, bj), score = H(bi, bj), tail = n - bi (a window without a positive cell: tail = n);  ratio = matches / ext_len
 *                 as float, 0 when ext_len is 0;  open = 1 iff the row is partial and tail <= max_tail
 * The repeat is x[lo .. lo + ext_len) for a forward slot and x[hi - ext_len .. hi) for a backward one.  open = 1 says that the repeat runs off the
 * read: copies is a LOWER BOUND.  An empty window (lo == hi) gives partial = 1, open = 1, zeros in ext, and no DP.
 * seqs / seq_off, the rows and the protocol are mtr_genotype_loci_device's; the call keeps nothing and drops nothing the batch or a run keeps.
 * Checked in the genotype's order up to its row limit; then MTR_ERR_BAD_ARG for a motif of more than 32 bases (the message names the locus: this
 * call aligns one extension per lane and nothing else) and for max_tail < 0.  There is no MTR_ERR_DP_TOO_LARGE: nothing is stored per cell.  Then
 * *out_rows = n_reads * n_loci and dst as there (cap_rows); a failed call writes nothing. */
typedef struct mtr_partial_dst {
    uint8_t *partial;      /* [R] */
    uint8_t *slot;         /* [R] 0 .. 3 */
    int32_t *flank_dist;   /* [R] */
    int32_t *window;       /* [R*2] lo, hi */
    int32_t *ext;          /* [R*6] ext_len, motif_bases, copies, matches, score, tail */
    float   *ratio;        /* [R] */
    uint8_t *open;         /* [R] */
    int64_t  cap_rows;
} mtr_partial_dst;   /* caller-owned DEVICE memory; row = read * n_loci + locus */
mtr_status mtr_genotype_partial_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist,
                                       int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail, const mtr_partial_dst *dst, int64_t *out_rows);

/* ---- partial genotype at catalogue scale: one seeded flank is a candidate ---------------------------------------------------------------------------
 * mtr_genotype_partial_device scans every read against every flank and writes a row per (read, locus).  This call returns exactly the rows that
 * call would write with partial = 1 - every column bit for bit - as a list sorted by (read, locus), and does no work and no allocation sized
 * reads x loci.  It is not an approximation:
 *   seeds       as the catalogue genotype defines them: K + 1 disjoint q-mers per pattern, m >= (K + 1) * q, q = seed_len in 8..16.
 *   candidate   (read, locus) where the read holds a seed of AT LEAST ONE of the locus' four slots (A, B, rc A, rc B).  A slot within K edits
 *               leaves one of its seeds in the read verbatim, so a pair that is no candidate has no slot within K and the dense call writes zeros
 *               for it.  (The catalogue genotype asks for both flanks of an orientation; a partial row needs one flank.)
 *   rows        for a candidate a seeded slot's hit F(.) is the flank search's own, over the whole read; an unseeded slot counts as dist > K.  On
 *               these four the genotype's pairing rule decides "spanning" - such a pair is no row - and otherwise the partial genotype's choice of
 *               slot, window, direction, motif, extension, tail, ratio and open apply verbatim.  A candidate with no slot within K is no row.
 *   columns     read [R], locus [R], and mtr_partial_dst's seven columns with R rows; partial is 1 throughout.
 * Two entry points, as the catalogue genotype's: the context keeps the result, the copy hands it out.
 * mtr_genotype_partial_catalog_device: checked in this order - the genotype's checks, its limit of 2^30 - 1 (read, locus) pairs included; a motif
 * of more than 32 bases, then max_tail < 0 (the partial genotype's); seed_len outside 8..16, then a flank shorter than (max_flank_dist + 1) *
 * seed_len, naming locus and side (the catalogue's).  There is no MTR_ERR_DP_TOO_LARGE.  MTR_ERR_OVERFLOW for 2^31 - 1 seed hits or more, or more
 * than 2^30 - 1 candidates.  On MTR_OK *out_rows = R, *out_candidates = the number of (read, locus) candidates verified, and the rows are kept; a
 * failed call keeps nothing and writes nothing.  The kept rows are this call's own: an upload of any kind and the next call of this kind (whatever
 * its outcome) discard them; mtr_genotype_catalog_device does not, and this call does not discard what that one kept.
 * mtr_genotype_partial_catalog_copy_device follows mtr_genotype_catalog_copy_device's rules: MTR_ERR_BAD_ARG if nothing is kept or dst is NULL;
 * MTR_ERR_OVERFLOW if rows.cap_rows < R, and then nothing is written; MTR_ERR_BAD_ARG if R > 0 and a column is NULL; else the columns are written
 * and the context's stream is synchronised before the call returns.  Two calls with the same arguments give byte-identical columns.
 * What the call is meant for is what the catalogue genotype is meant for: seeds that are rare in the reads.  A read's hits are compared pairwise to
 * find its candidates (quadratic in the read's hits); with 4^seed_len well above the catalogue's 4 * (max_flank_dist + 1) * n_loci seeds -
 * seed_len >= 12 for 100 000 loci - a 2 kb read has tens to hundreds of hits; at seed_len = 8 a catalogue of more than a few thousand loci makes
 * every position a hit of several entries and the call slower than the dense one.  Choose the largest seed_len the flanks admit. */
typedef struct mtr_partial_catalog_dst {
    int32_t *read;           /* [R] */
    int32_t *locus;          /* [R] */
    mtr_partial_dst rows;    /* the partial genotype's columns, R rows; cap_rows is the capacity of all nine */
} mtr_partial_catalog_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_genotype_partial_catalog_device(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist,
                                               int32_t seed_len, int32_t gain, int32_t mismatch, int32_t indel, int32_t max_tail,
                                               int64_t *out_rows, int64_t *out_candidates);
mtr_status mtr_genotype_partial_catalog_copy_device(mtr_ctx *ctx, const mtr_partial_catalog_dst *dst);

/* ---- a prepared locus catalogue: what depends on the loci alone, built on the GPU once and used by every batch --------------------------------
 * A locus list is fixed for a run while the reads come batch after batch; the two catalogue calls above rebuild per call everything that
 * depends on the loci alone (the seed index, the slots' masks, the motif tables).  An mtr_catalog holds all of that in DEVICE memory, made once;
 * the two prepared calls take it in place of the loci and return, bit for bit, what the text-taking calls return for the same loci, seed_len and
 * max_flank_dist on the same batch.
 * mtr_catalog_create: seqs / seq_off, n_loci, max_flank_dist, seed_len as mtr_genotype_catalog_device takes them.  It needs NO uploaded batch: ctx
 * gives the device, the stream and the place of mtr_last_error.  A run in flight on ctx ends first.  It makes every check of the text-taking
 * calls that does not depend on the reads or the scores, in their order and with their status and message for the same argument: n_loci < 1,
 * seqs or seq_off NULL, more than 2^29 - 1 loci, a decreasing seq_off, more than 2^30 - 1 motifs or motif bases, a motif's length outside
 * 1..499 or a byte of it outside ACGT, a flank's length outside 1..64 or a byte of it outside ACGT, max_flank_dist < 0, seed_len outside 8..16,
 * a flank shorter than (max_flank_dist + 1) * seed_len.  A motif of more than 32 bases is legal here (mtr_catalog_info names the first);
 * the prepared partial call refuses such a catalogue.  MTR_ERR_OVERFLOW if 4 * n_loci * (max_flank_dist + 1) seeds exceed 2^31 - 1; MTR_ERR_OOM /
 * MTR_ERR_HIP as elsewhere ("the seed table is full" is MTR_ERR_HIP: the table's probes are bounded).  On anything but MTR_OK *out is NULL.
 * The host reads only seq_off (lengths); every table that depends on a base is computed on the device from one upload of seqs: the slots'
 * patterns, masks and seeds, the entries sorted by (code, slot) by a stable radix sort and made distinct, the runs, the filter, the table, the
 * motif tables.  The entries, the filter and everything a probe of the table returns equal what the text-taking calls build on the host; the
 * places of the codes in the table may differ.
 * Lifetime and sharing: the catalogue is immutable once create returns, and the device is synchronised before it returns.  Any context on the
 * same device may use it, several at once (each on its own stream), whether or not the creating context still exists; a context on another
 * device gets MTR_ERR_BAD_ARG.  No upload, run or genotype call changes it.  mtr_catalog_destroy frees it (NULL: a no-op); no call may be using it.
 * mtr_genotype_catalog_prepared_device / mtr_genotype_partial_catalog_prepared_device: checked in this order - ctx, cat, the out pointers; no
 * batch uploaded; n_reads x n_loci beyond the text-taking calls' limits; (the catalogue genotype only) the WrapDPsize test, MTR_ERR_DP_TOO_LARGE;
 * the scores; (the partial call only) a motif of more than 32 bases, naming the locus, then max_tail < 0 - each with the text-taking call's
 * message.  Whatever the outcome, the rows the context kept of the same kind of call are discarded, as the text-taking calls discard them; on
 * MTR_OK the rows are kept in the context exactly as mtr_genotype_catalog_device / mtr_genotype_partial_catalog_device keep them, and
 * mtr_genotype_catalog_copy_device / mtr_genotype_partial_catalog_copy_device hand them out.  Nothing sized by the catalogue is built by these
 * calls.  What the test switches of a call decide from the lengths - which motif slots run a lane each, which flank words are launched - goes into
 * the context's own buffers: the lane-slot lists are derived and uploaded once per (catalogue, MTR_TEST_MOTIF_LANE_MAX) and kept in the context
 * until another catalogue, another value or a text-taking genotype call takes their place, so batch after batch on one catalogue sends nothing
 * sized by it.  MTR_ABI_VERSION is unchanged by these entries: look for them by symbol. */
typedef struct mtr_catalog mtr_catalog;
typedef struct mtr_catalog_info {
    int32_t n_loci, max_flank_dist, seed_len;
    int32_t filter_bits;          /* the filter has 2^filter_bits bits */
    int64_t entries;              /* distinct (code, slot) pairs */
    int64_t distinct_codes;
    int64_t table_slots;          /* a power of two >= 2 * distinct_codes, at least 64 */
    int64_t first_long_motif;     /* the first locus whose motif exceeds 32 bases, or -1 */
    int64_t device_bytes;         /* what the catalogue holds in device memory */
} mtr_catalog_info;
mtr_status mtr_catalog_create(mtr_ctx *ctx, const char *seqs, const int64_t *seq_off, int32_t n_loci, int32_t max_flank_dist, int32_t seed_len,
                              mtr_catalog **out);
void mtr_catalog_destroy(mtr_catalog *cat);
mtr_status mtr_catalog_info_get(const mtr_catalog *cat, mtr_catalog_info *info);
mtr_status mtr_genotype_catalog_prepared_device(mtr_ctx *ctx, const mtr_catalog *cat, int32_t gain, int32_t mismatch, int32_t indel,
                                                int64_t *out_rows, int64_t *out_candidates);
mtr_status mtr_genotype_partial_catalog_prepared_device(mtr_ctx *ctx, const mtr_catalog *cat, int32_t gain, int32_t mismatch, int32_t indel,
                                                        int32_t max_tail, int64_t *out_rows, int64_t *out_candidates);

/* ---- allele calls: the genotype's rows of a locus ranked and split ---------------------------------------------------------------------------------
 * "Which alleles does the sample carry at this locus?"  The genotype answers per read; this call reduces every read that spans a locus to one or
 * two values.  The input is genotype rows in DEVICE memory, row = read * n_loci + locus, n_reads >= 1, n_loci >= 1, n_reads * n_loci <= 2^31 - 1:
 * what one mtr_genotype_loci_device call wrote, or several calls' rows concatenated along the read axis (the batches of a file walk go in as one
 * input; n_reads is an argument).  The call needs no uploaded batch and touches nothing the context keeps of one.
 * The definition, for the parameters measure, min_ratio, min_support, min_percent, min_sep (mtr_allele_params):
 *   supporting row   a row supports its locus iff spanning == 1 and (window[1] == window[0] or ratio >= min_ratio), the comparison made in float32;
 *                    a row with spanning == 0 is skipped whatever its other columns hold
 *   value            v = fields[3] (measure = MTR_ALLELE_COPIES) or window[1] - window[0] (MTR_ALLELE_BASES); v < 0 in a supporting row is
 *                    MTR_ERR_BAD_ARG, the message names the row (the smallest such row), nothing is written
 *   support list     the supporting rows of a locus sorted by (v, read) ascending; locus l has S_l of them, S = sum S_l; support_off[n_loci + 1]
 *                    is the prefix of S_l, value[S] and read[S] hold the sorted lists, one locus after the other
 *   med, sad         for the sorted values v[0 .. S_l) of one locus: med(i, j) = v[i + (j - i - 1) / 2], the lower median of the segment [i, j);
 *                    sad(i, j) = sum over t in [i, j) of |v[t] - med(i, j)|, as int64; cost1 = sad(0, S_l)
 *   admissible       a split k, 1 <= k < S_l, is admissible iff v[k - 1] < v[k] (reads of one value are never separated), min(k, S_l - k) >=
 *                    min_support, min(k, S_l - k) * 100 >= min_percent * S_l (in int64), and med(k, S_l) - med(0, k) >= min_sep
 *   cost2(k)         = sad(0, k) + sad(k, S_l)
 *   S_l < min_support (S_l == 0 too)   zygosity 0, call (0, 0), call_support (0, 0), cost (0, 0), allele 0 for the locus' entries; value and read
 *                                      are still written
 *   no admissible k                    zygosity 1, call (med(0, S_l), med(0, S_l)), call_support (S_l, 0), cost (cost1, cost1), allele 0
 *   an admissible k exists             zygosity 2, k = the admissible split of smallest cost2, the smallest such k on a tie: call (med(0, k),
 *                                      med(k, S_l)), call_support (k, S_l - k), cost (cost1, cost2(k)), allele[t] = 0 for t < k and 1 from k on
 * Every output is an exact integer and none depends on the order in which the device worked.
 * rows is the genotype's own struct read as INPUT: cap_rows >= n_reads * n_loci; only spanning, window, fields and ratio are read, the other
 * three pointers may be NULL.  wait_stream is the stream that wrote the rows, handled as mtr_upload_batch_device handles it.
 * Checked in this order, each MTR_ERR_BAD_ARG with mtr_last_error naming the offender: NULL ctx, out_support, rows or prm;  n_reads < 1, n_loci < 1,
 * more than 2^31 - 1 rows;  measure, min_ratio (0 <= min_ratio <= 1, not NaN), min_support (>= 1), min_percent (0..50), min_sep (>= 1) out of
 * range, in this order;  a NULL needed input column or cap_rows too small;  a needed input column that is not device memory of the context's GPU
 * or runs past its allocation.  Then the rows are counted: *out_support = S, and the negative value's error.  Then, as the report calls: dst ==
 * NULL: MTR_OK with the size only;  cap_loci < n_loci or cap_support < S: MTR_ERR_OVERFLOW, nothing written;  a NULL destination column:
 * MTR_ERR_BAD_ARG (value, read and allele may be NULL only when S == 0);  else the columns are written and the context's stream synchronised
 * before the call returns.  A failed call writes nothing into dst. */
#define MTR_ALLELE_COPIES 0
#define MTR_ALLELE_BASES 1
typedef struct mtr_allele_params {
    int32_t measure;       /* MTR_ALLELE_COPIES or MTR_ALLELE_BASES */
    float   min_ratio;     /* the smallest ratio a row with a non-empty window may have */
    int32_t min_support;   /* the fewest reads an allele needs */
    int32_t min_percent;   /* the smaller allele's least share of the locus' supporting reads, in percent */
    int32_t min_sep;       /* the least distance between the two alleles' values */
} mtr_allele_params;
typedef struct mtr_allele_calls_dst {
    int64_t *support_off;   /* [n_loci + 1] */
    int32_t *value;         /* [S] */
    int32_t *read;          /* [S] */
    uint8_t *allele;        /* [S] */
    uint8_t *zygosity;      /* [n_loci] */
    int32_t *call;          /* [n_loci * 2] */
    int32_t *call_support;  /* [n_loci * 2] */
    int64_t *cost;          /* [n_loci * 2] cost1, cost2 */
    int64_t  cap_loci;
    int64_t  cap_support;
} mtr_allele_calls_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_call_alleles_device(mtr_ctx *ctx, const mtr_genotypes_dst *rows, int64_t n_reads, int32_t n_loci,
                                   const mtr_allele_params *prm, void *wait_stream,
                                   const mtr_allele_calls_dst *dst, int64_t *out_support);
/* mtr_call_alleles_rows_device: the same call - the same definition, parameters, outputs and protocol - over a LIST of n_rows >= 0 genotype rows in
 * any order, each naming its read and locus in two more DEVICE columns, row_read [n_rows] and row_locus [n_rows] (int32): what
 * mtr_genotype_catalog_copy_device wrote, or several batches' rows concatenated column by column after the batch's first read's index was added to
 * its read column.  A row's read and locus come from these columns instead of row / n_loci and row % n_loci; rows->cap_rows >= n_rows.  A (read,
 * locus) without a row is a pair that does not span.  Checked as above with n_rows (0 .. 2^31 - 1) in place of the dense shape and NULL index
 * columns refused when n_rows > 0; then, on the device and before any kernel is given dst, MTR_ERR_BAD_ARG for a row whose locus is outside
 * 0 .. n_loci - 1 or whose read is negative, and for a (locus, read) that more than one row names - the rank's keys (value, read) are distinct
 * only if it is unique (mtr_last_error names the row, or the pair); nothing is written then. */
mtr_status mtr_call_alleles_rows_device(mtr_ctx *ctx, const mtr_genotypes_dst *rows, const int32_t *row_read, const int32_t *row_locus,
                                        int64_t n_rows, int32_t n_loci, const mtr_allele_params *prm, void *wait_stream,
                                        const mtr_allele_calls_dst *dst, int64_t *out_support);

/* ---- allele consensus: each called allele's sequence by vote --------------------------------------------------------------------------------------
 * A call says "19 and 42 copies"; this says what those alleles are: the consensus of the reads that support an allele, interruptions included.
 * The reference has nothing of this kind; the definition is this project's own.  Two calls.
 *
 * mtr_extract_windows_device: the oriented windows of n_rows >= 0 genotype rows out of the RESIDENT batch, before the next upload replaces it.
 * row_read [n_rows] (indices into the resident batch: before a joining offset is added), orientation [n_rows] and window [n_rows * 2] are DEVICE
 * columns as mtr_genotype_catalog_copy_device writes them.  Row r's oriented window is win_bases[win_off[r] .. win_off[r + 1]), codes 0..3: the
 * read's bases [lo, hi) for orientation 0, their reverse complement for orientation 1 - every window reads in the locus' direction.
 * *out_bases = T, the windows' bases in all.  Checked in this order, MTR_ERR_BAD_ARG with mtr_last_error naming the offender: NULL ctx or
 * out_bases; no batch uploaded; n_rows outside 0..2^31 - 1; a NULL input column with n_rows > 0; an input column that is not device memory of the
 * context's GPU or runs past its allocation; then, on the device and before any kernel is given dst, a row whose read is outside the batch or
 * whose window is outside its read (the smallest such row).  Then dst == NULL: MTR_OK with T only; cap_rows < n_rows or cap_bases < T:
 * MTR_ERR_OVERFLOW, nothing written; a NULL win_off, or a NULL win_bases with T > 0: MTR_ERR_BAD_ARG; else the columns are written and the
 * context's stream synchronised before the call returns.  wait_stream is the stream that wrote the rows, handled as mtr_upload_batch_device
 * handles it.  Several batches' windows are joined by concatenating win_bases and shifting each batch's win_off by the bases before it.
 *
 * mtr_allele_consensus_device: needs no uploaded batch and touches nothing a batch or a run left.  src, all DEVICE memory: the joined rows'
 * row_read and row_locus [n_rows], ascending by (read, locus) and distinct - checked on the device, MTR_ERR_BAD_ARG names the first row out of
 * order; their windows win_off [n_rows + 1], win_bases [n_bases]; of the allele calls over the same rows support_off [n_loci + 1], read
 * [n_support], allele [n_support], zygosity [n_loci].  A support entry (locus l, read q) finds its row by bisection over (read, locus); an entry
 * without a row is MTR_ERR_BAD_ARG naming the entry, nothing is written.  band_extra in 0..MTR_CONS_MAX_EXTRA.
 * The definition:
 *   alleles     allele index A = 2 * locus + a, a in {0, 1}.  Zygosity 0 has no alleles, zygosity 1 allele 0 only, zygosity 2 both.  The members of
 *               an allele are the locus' support entries with allele == a, in list order (ascending (value, read)): n_A of them.  An allele
 *               without a member is no allele
 *   backbone    the member at position (n_A - 1) / 2 of that order - the entry whose value is the call; B is its oriented window, m = |B|
 *   aligned     every other member, with window W, n = |W|, is aligned to B unless it is skipped: n > MTR_CONS_MAX_WINDOW, m >
 *               MTR_CONS_MAX_WINDOW, or |m - n| + 2 * band_extra + 1 > MTR_CONS_MAX_BAND.  Skipped members are counted and vote nothing
 *   banded D    cells (i, j), 0 <= i <= n, 0 <= j <= m, exist iff dlo <= j - i <= dhi, dlo = min(0, m - n) - band_extra, dhi = max(0, m - n) +
 *               band_extra; other cells are infinite.  D(0, 0) = 0; else D(i, j) is the minimum of diag = D(i-1, j-1) + (W[i-1] != B[j-1]),
 *               up = D(i-1, j) + 1, left = D(i, j-1) + 1, and the cell's direction is the first of diag, up, left that attains it.  The band is
 *               part of the definition, not an approximation of something else
 *   votes       the walk from (n, m) to (0, 0) by the directions: diag at (i, j): base[j][W[i-1]] += 1; left at (i, j): del[j] += 1; a maximal
 *               run of up steps at column j is an insertion after backbone position j (j = 0: before the first base), whose bases vote in read
 *               order, ins[j][k][W[i0 + k]] += 1 for k < MTR_CONS_INS_SLOTS; further bases of the run vote nothing.  The backbone votes
 *               base[j][B[j-1]] += 1 for every j.  N = 1 + the aligned members
 *   emission    for j = 0 .. m: if j >= 1, c* = the base of most votes in base[j] - among tied bases the backbone's if it is one of them, else
 *               the lowest code - is emitted with votes = base[j][c*] unless del[j] > base[j][c*]; then the insertion slots k = 0, 1, .. after
 *               j: with tot = sum over c of ins[j][k][c] and mx its maximum (lowest code on a tie) slot k is emitted with votes = mx iff mx > N -
 *               tot; the first slot not emitted ends the junction.  Ties go to the backbone's state everywhere
 * Every output is an exact integer and none depends on the order in which the device worked.
 * Outputs, one group per allele index, G = 2 * n_loci: cons_off [G + 1] (an allele that is none has an empty span), bases [T] (codes), votes [T],
 * backbone_read (-1 without an allele), backbone_len, members, aligned, skipped [G] each.  *out_bases = T.  Checked in this order, each
 * MTR_ERR_BAD_ARG naming the offender: NULL ctx, out_bases or src; n_loci < 1 or above 2^30 - 1, n_rows, n_support or n_bases outside 0..2^31 - 1;
 * band_extra; a NULL input column that would be read; an input column that is not device memory of the context's GPU or runs past its
 * allocation; then on the device the rows' order, the offset columns (ascending from 0 to n_bases / n_support, no window above 2^30 bases), a
 * zygosity above 2, an entry without a row, an allele column that is not 0 .. 0 1 .. 1 within a locus.  Then the votes and the emission lengths are
 * computed, and as mtr_call_alleles_rows_device: dst == NULL: MTR_OK with T only; cap_alleles < G or cap_bases < T: MTR_ERR_OVERFLOW, nothing
 * written; a NULL destination column (bases and votes may be NULL only when T == 0): MTR_ERR_BAD_ARG; else the columns are written and the
 * context's stream synchronised before the call returns.  A failed call writes nothing into dst.  MTR_ABI_VERSION is unchanged by these
 * entries: look for them by symbol. */
#define MTR_CONS_MAX_WINDOW 16384
#define MTR_CONS_MAX_BAND 256
#define MTR_CONS_INS_SLOTS 4
#define MTR_CONS_MAX_EXTRA 64
typedef struct mtr_windows_dst {
    int64_t *win_off;       /* [n_rows + 1] */
    uint8_t *win_bases;     /* [T] */
    int64_t  cap_rows;
    int64_t  cap_bases;
} mtr_windows_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_extract_windows_device(mtr_ctx *ctx, const int32_t *row_read, const uint8_t *orientation, const int32_t *window, int64_t n_rows,
                                      void *wait_stream, const mtr_windows_dst *dst, int64_t *out_bases);
typedef struct mtr_consensus_src {
    const int32_t *row_read;     /* [n_rows] */
    const int32_t *row_locus;    /* [n_rows] */
    const int64_t *win_off;      /* [n_rows + 1] */
    const uint8_t *win_bases;    /* [n_bases] */
    const int64_t *support_off;  /* [n_loci + 1] */
    const int32_t *read;         /* [n_support] */
    const uint8_t *allele;       /* [n_support] */
    const uint8_t *zygosity;     /* [n_loci] */
    int64_t n_rows, n_bases, n_support;
    int32_t n_loci;
} mtr_consensus_src;   /* DEVICE memory, read only */
typedef struct mtr_consensus_dst {
    int64_t *cons_off;       /* [2 * n_loci + 1] */
    uint8_t *bases;          /* [T] */
    int32_t *votes;          /* [T] */
    int32_t *backbone_read;  /* [2 * n_loci] */
    int32_t *backbone_len;   /* [2 * n_loci] */
    int32_t *members;        /* [2 * n_loci] */
    int32_t *aligned;        /* [2 * n_loci] */
    int32_t *skipped;        /* [2 * n_loci] */
    int64_t  cap_alleles;
    int64_t  cap_bases;
} mtr_consensus_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_allele_consensus_device(mtr_ctx *ctx, const mtr_consensus_src *src, int32_t band_extra, void *wait_stream,
                                       const mtr_consensus_dst *dst, int64_t *out_bases);

/* ---- qualities of the resident batch, their windows, and the quality-weighted allele consensus ---------------------------------------------------
 * The allele consensus gives every base one vote, whether the basecaller called it with Q3 or Q40.  These entries carry the FASTQ's own
 * qualities from the file to the vote.  Stored qualities are Phred values 0..MTR_QUAL_MAX, one byte per base, in a buffer the context owns: read
 * r's at the exclusive sum of the lengths of the reads before it.  They belong to the resident batch: every upload replaces or drops them.
 *
 * mtr_keep_qualities: a sticky option of the context, off by default (on != 0: on).  While it is on, mtr_upload_fastq_device, its _in_file and
 * its _window form also gather each read's quality line, after the upload itself has succeeded: the stored value of a byte b is min(MTR_QUAL_MAX,
 * max(0, b - 33)).  An upload made with the option off, and an upload of FASTA, text, codes or a packed image, leaves no qualities.
 * mtr_attach_qualities_device: the caller's Phred values (NOT ASCII) for the resident batch, whatever uploaded it: read i's are d_qual[offsets[i]
 * .. offsets[i] + lens[i]), d_qual DEVICE memory of n_bytes bytes, offsets [n_reads] on the HOST; a value above MTR_QUAL_MAX is stored as
 * MTR_QUAL_MAX.  MTR_ERR_BAD_ARG naming the offender: no batch resident; d_qual or offsets NULL, d_qual not device memory of the context's GPU or
 * n_bytes running past its allocation; a read whose span leaves 0..n_bytes (the smallest such read).  A refused call leaves the qualities as
 * they were.  mtr_qualities_resident: *out_bytes = the stored bytes, 0 when there are none.
 *
 * mtr_extract_window_qualities_device: the byte-for-byte companion of mtr_extract_windows_device - the same arguments, the same checks in the
 * same order (behind "no batch uploaded": no qualities resident, MTR_ERR_BAD_ARG "no qualities resident"), the same T.  Row r's values are
 * dst_qual[win_off[r] .. win_off[r + 1]) with mtr_extract_windows_device's win_off: the read's values [lo, hi) for orientation 0, the same
 * reversed - not complemented - for orientation 1, so that value k belongs to base k of the oriented window.  dst_qual == NULL: MTR_OK with T
 * only; cap < T: MTR_ERR_OVERFLOW, nothing written.
 *
 * mtr_allele_consensus_quality_device: mtr_allele_consensus_device with weighted votes.  src and dst are its structs, win_qual [n_bases] is
 * DEVICE memory aligned with src->win_bases, the outputs are its eight columns with votes holding weight sums.  The alleles, the backbone, the
 * skip rule, the banded D and its directions, the tie rules, the protocol and the checks with their order are exactly its own: the alignment
 * is not weighted.  Two refusals come behind band_extra: qual_cap outside 1..MTR_CONSQ_MAX_CAP, and n_support * qual_cap >= 2^31 (the sums are
 * int32); a NULL win_qual with n_bases > 0 is a NULL input column, and its memory is checked behind win_bases'.
 * The definition:
 *   weights     w(q) = min(max(q, 1), qual_cap).  For a member with window W of n bases, omega[i] = w(the quality of W[i]); omegaB is the same
 *               for the backbone.  The gap weight gamma(i) at boundary i of a window, 0 <= i <= n, is min(omega[i-1], omega[i]) where both exist,
 *               the one that exists at the ends, 1 for an empty window; gammaB is the backbone's
 *   the path    the walk from (n, m) to (0, 0) visits every column j = 0 .. m, in column j the rows lo_j .. hi_j: L_j = hi_j - lo_j is its run of up
 *               steps there, which inserts W[lo_j .. hi_j) after backbone position j, and it leaves column j >= 1 from (lo_j, j) by diag or left
 *   votes       of an aligned member: diag from (i, j): base[j][W[i-1]] += omega[i-1]; left from (i, j): del[j] += gamma(i); ins[j][k][W[lo_j + k]]
 *               += omega[lo_j + k] for k < min(L_j, MTR_CONS_INS_SLOTS); and if L_j < MTR_CONS_INS_SLOTS: end[j][L_j] += gamma(hi_j) - the member
 *               says "nothing more here from slot L_j on" with the weight of the boundary where that nothing is.  Of the backbone:
 *               base[j][B[j-1]] += omegaB[j-1] for every j
 *   emission    for j = 0 .. m: if j >= 1, c* = the base of the largest base[j] - among tied bases the backbone's if it is one of them, else the
 *               lowest code - is emitted with votes = base[j][c*] unless del[j] > base[j][c*]; then the insertion slots k = 0, 1, .. after j: with
 *               none_k = gammaB(j) + the sum of end[j][L] over L <= k, and mx the maximum over c of ins[j][k][c] (lowest code on a tie), slot k is
 *               emitted with votes = mx iff mx > none_k; the first slot not emitted ends the junction
 * Every output is an exact integer and none depends on the order in which the device worked.  With qual_cap = 1 every weight is 1, none_k is
 * N - tot, and the result is mtr_allele_consensus_device's in all eight columns, whatever the qualities.  With one constant quality c <=
 * qual_cap and no empty window among the members and backbones, the bases are the unweighted ones and votes c times the unweighted votes.
 * MTR_ABI_VERSION is unchanged by these entries: look for them by symbol. */
#define MTR_QUAL_MAX 93
#define MTR_CONSQ_MAX_CAP 93
mtr_status mtr_keep_qualities(mtr_ctx *ctx, int32_t on);
mtr_status mtr_attach_qualities_device(mtr_ctx *ctx, const uint8_t *d_qual, int64_t n_bytes, const int64_t *offsets, void *wait_stream);
mtr_status mtr_qualities_resident(const mtr_ctx *ctx, int64_t *out_bytes);
mtr_status mtr_extract_window_qualities_device(mtr_ctx *ctx, const int32_t *row_read, const uint8_t *orientation, const int32_t *window, int64_t n_rows,
                                               void *wait_stream, uint8_t *dst_qual, int64_t cap, int64_t *out_bases);
mtr_status mtr_allele_consensus_quality_device(mtr_ctx *ctx, const mtr_consensus_src *src, const uint8_t *win_qual, int32_t band_extra, int32_t qual_cap,
                                               void *wait_stream, const mtr_consensus_dst *dst, int64_t *out_bases);

/* ---- window structure: compound loci counted segment by segment ---------------------------------------------------------------------------------
 * A genotype row's `copies` is one count for one motif, taken from a LOCAL alignment; a compound locus - HTT's (CAG)n CAACAG CCGCCA (CCG)m - and
 * the interruptions a consensus carries need the GLOBAL alignment of an oriented window to an ORDERED LIST of motifs, each repeated zero or more
 * whole times, reported per segment.  The reference has nothing of this kind; the definition is this project's own.  It applies unchanged to the
 * windows of mtr_extract_windows_device and to the sequences of mtr_allele_consensus_device: both are off [N + 1], bases [T], codes 0..3.
 * The definition:
 *   structure   motifs M_0 .. M_{S-1} over ACGT, 1 <= S <= MTR_WS_MAX_SEGMENTS = 4, U_s = |M_s| >= 1, W = sum U_s.  Limit: S <= 2 and W <= 32, or
 *               S <= 4 and W <= 16 (the per-segment counters are 16-bit fields: two fit one register, four a register pair, and a cell is
 *               carried in registers, one DP per lane).  The columns are flat, c = 0 .. W-1; seg(c), first(s) and last(s) name a column's
 *               segment and a segment's end columns; m[c] is the motif base of column c.  A state START stands for "no motif base consumed yet"
 *   window      y[0 .. n), codes 0..3, n <= MTR_WS_MAX_WINDOW = 16384.  Scores G (gain), MM (mismatch), D (indel) in the search's ranges
 *   predecessors of a column, in this order: for c != first(seg(c)): [c - 1]; for c = first(s): [last(s-1), last(s-2), .., last(0), START,
 *               last(s)] - the segment's own wrap comes last
 *   cells       rows i = 0 .. n.  H(i, START) = -D * i.  For a column c, H(i, c) is the largest of these candidates: sub (i >= 1), for each
 *               predecessor p in order: H(i-1, p) + (G if y[i-1] == m[c] else -MM); up (i >= 1): H(i-1, c) - D; left, for each predecessor p in
 *               order: H(i, p) - D.  Row 0 has left only.  The cell's predecessor is the FIRST candidate in that order (subs, then up, then
 *               lefts) that attains the maximum.  A cell with no finite candidate is minus infinity
 *   fixpoint    the lefts make a row cyclic through the wrap, and H is the fixpoint.  Two sweeps reach it: sweep 1 computes the row without the
 *               wrap's left; sweep 2, per segment: if H(i, last(s)) - D is STRICTLY greater than H(i, first(s)) it replaces it, and the
 *               improvement runs on by lefts while it stays strictly greater.  Once round a segment by lefts costs U_s * D > 0, so sweep 2 never
 *               changes last(s) and needs no third sweep.  The wrap is the last left candidate and subs and up come before lefts, so "strictly
 *               greater" is exactly the priority rule
 *   carried     with a cell, from its predecessor: copies[s], plus 1 when a sub or left lands on last(s); matches[s], plus 1 on a matching sub
 *               in segment s; entry[s], set when a step lands on first(s) from any predecessor other than last(s): to i - 1 for a sub, to i for
 *               a left.  A copy made only of lefts strictly loses, so every count is at most n <= 16384 and fits 16 bits
 *   end         the best of H(n, e) over e in [last(S-1), .., last(0), START], the first in that order that attains the maximum.  Only whole
 *               copies exist: a segment is entered at first and left from last
 * Columns per window w: seg [N * 4 * 4] = start, end, copies, matches per segment - going from s = S-1 down with nxt = n, a segment with copies >
 * 0 spans [entry[s], nxt) and sets nxt = entry[s]; a segment with no copies is (nxt, nxt, 0, 0); segments >= S are zeros; bases before the first
 * used segment belong to none.  score [N] = H of the end.  ratio [N] = float(sum matches) / n, or 0 for n == 0.  skipped [N] = 1 for n >
 * MTR_WS_MAX_WINDOW; such a window is zeros elsewhere.  n == 0 is score 0, all zeros, and no DP.  Every output but ratio is an exact integer,
 * and none depends on where or in which order the device worked.
 *
 * mtr_window_structure_device: motifs, motif_off and struct_off [n_structs + 1] are HOST arrays: structure k is motifs struct_off[k] ..
 * struct_off[k + 1], motif j the bytes motifs[motif_off[j] .. motif_off[j + 1]).  win_off [n_windows + 1], win_bases [n_bases] and win_struct
 * [n_windows] (int32, the window's structure) are DEVICE columns.  The call needs no uploaded batch and touches nothing a batch, a run or another
 * call keeps; its buffers are its own.  Checked in this order, each MTR_ERR_BAD_ARG with mtr_last_error naming the offender: a NULL ctx; NULL
 * motifs, motif_off or struct_off; a NULL device column that would be read, a NULL dst or destination column (with n_windows > 0); n_structs
 * outside 1..2^24, n_windows outside 0..2^31 - 1, n_bases negative; the scores (gain 1..5, mismatch and indel 1..3); struct_off, then motif_off,
 * decreasing; then, each over all structures before the next: a structure of 0 or more than 4 motifs, a motif of length 0, the column limit, a
 * byte that is none of ACGT; a device column that is not memory of the context's GPU or runs past its allocation; then on the device, the
 * smallest offender of each kind: win_off not ascending from 0 to n_bases, a win_struct outside 0 .. n_structs - 1, a base code above 3.  Then
 * cap_windows < n_windows: MTR_ERR_OVERFLOW.  Else the columns are written and the context's stream synchronised before the call returns.  A
 * failed call writes nothing into dst.  wait_stream is the stream that wrote the columns, handled as mtr_upload_batch_device handles it.
 * MTR_ABI_VERSION is unchanged by this entry: look for it by symbol. */
#define MTR_WS_MAX_SEGMENTS 4
#define MTR_WS_MAX_WINDOW 16384
typedef struct mtr_window_structure_dst {
    int32_t *seg;           /* [n_windows * 4 * 4]: start, end, copies, matches per segment */
    int32_t *score;         /* [n_windows] */
    float   *ratio;         /* [n_windows] */
    uint8_t *skipped;       /* [n_windows] */
    int64_t  cap_windows;
} mtr_window_structure_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_window_structure_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, const int32_t *struct_off, int32_t n_structs,
                                       const int64_t *win_off, const uint8_t *win_bases, const int32_t *win_struct, int64_t n_windows, int64_t n_bases,
                                       int32_t gain, int32_t mismatch, int32_t indel, void *wait_stream, const mtr_window_structure_dst *dst);

/* ---- window edits: each interruption by segment, copy and column ----------------------------------------------------------------------------------
 * The window structure counts; it does not say WHICH copy of a segment deviates, at which motif base, or how - the CAA inside a CAG tract, the
 * AGG inside CGG.  The window edits list it.  Structure, window, scores, cells, fixpoint, predecessor order and end are the window structure's,
 * unchanged, and so are the limits: S <= 2 and W <= 32, or S <= 4 and W <= 16; n <= MTR_WS_MAX_WINDOW.  The predecessor order makes the
 * alignment path a function of the window alone, so the list is too.  The definition:
 *   path        the chain of predecessors from the end back to START, read FORWARD.  Every step lands on a cell (i, c), s = seg(c): a sub step
 *               from (i-1, p), an up step from (i-1, c), a left step from (i, p)
 *   copy index  k = (the number of steps up to and including this one that landed on first(s) by sub or left) - 1.  Only whole copies exist,
 *               so every copy begins with such a landing and k runs over 0 .. copies[s] - 1 in window order.  An up step belongs to the copy
 *               its column was last landed in (it lands on first(s) by neither sub nor left, so the count does not move)
 *   edits       in path order: kind 0, substitution: a sub step with y[i-1] != m[c]; pos = i - 1, base = y[i-1].  kind 1, insertion: an up
 *               step - a window base with no motif base, after motif base c of copy k; pos = i - 1, base = y[i-1].  kind 2, deletion: a left
 *               step - a motif base with no window base; pos = i, base = m[c].  Matching subs are no edits, nor are the rows spent in START
 *               before the first used segment
 *   row         per edit int32 [6] (MTR_WE_FIELDS): pos, segment, copy, column (c - first(s)), kind, base
 *   per window  seg, score and skipped as mtr_window_structure_device returns them for the same input, bit for bit.  An empty or a skipped
 *               window has no edits
 *   invariants  per window and segment s, since every copy lands on each of its U_s columns once by sub or left, and every row of a segment's
 *               span is consumed by one sub or one up:
 *                 copies * U_s == matches + #kind 0 + #kind 2          end - start == matches + #kind 0 + #kind 1
 * Columns: off [N + 1] int64 (window w's edits are rows off[w] .. off[w + 1]), edits [T * 6] int32 with T = off[N], seg [N * 4 * 4], score [N],
 * skipped [N].  None depends on where or in which order the device worked.
 *
 * mtr_window_edits_device computes into buffers of the context's own and keeps them (compute, then copy, as mtr_genotype_catalog_device and
 * mtr_genotype_catalog_copy_device); nothing of a batch, a run or another call is touched.  Its arguments are mtr_window_structure_device's
 * without dst, checked in the same order with the same words (out_edits counts among the columns that must not be NULL); *out_edits = T.  The
 * decisions of every cell are kept only while a ROUND of windows is worked on: at most MTR_WE_SCRATCH_BYTES of them at a time (or one
 * wavefront's 64 windows, if those alone need more) - up to 12 bytes a row and window.  The buffer that holds them is the context's, grown to the
 * largest round it has had and kept, like its other buffers, until mtr_destroy: transient is what it holds, not the allocation.  mtr_window_edits_copy_device copies what the last
 * successful call kept, device to device, into caller-owned DEVICE memory: MTR_ERR_BAD_ARG without such a call or with a NULL dst or column that
 * would be written; cap_windows < N or cap_edits < T: MTR_ERR_OVERFLOW, and nothing is written.  The context's stream is synchronised before
 * either returns.  MTR_ABI_VERSION is unchanged by these entries: look for them by symbol. */
#define MTR_WE_FIELDS 6
#define MTR_WE_SCRATCH_BYTES ((int64_t)1 << 29)
typedef struct mtr_window_edits_dst {
    int64_t *off;           /* [n_windows + 1] */
    int32_t *edits;         /* [n_edits * 6]: pos, segment, copy, column, kind, base */
    int32_t *seg;           /* [n_windows * 4 * 4] */
    int32_t *score;         /* [n_windows] */
    uint8_t *skipped;       /* [n_windows] */
    int64_t  cap_windows;
    int64_t  cap_edits;
} mtr_window_edits_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_window_edits_device(mtr_ctx *ctx, const char *motifs, const int64_t *motif_off, const int32_t *struct_off, int32_t n_structs,
                                   const int64_t *win_off, const uint8_t *win_bases, const int32_t *win_struct, int64_t n_windows, int64_t n_bases,
                                   int32_t gain, int32_t mismatch, int32_t indel, void *wait_stream, int64_t *out_edits);
mtr_status mtr_window_edits_copy_device(mtr_ctx *ctx, const mtr_window_edits_dst *dst);

/* ---- sequence allele calls: pairwise window distances, a two-medoid split ------------------------------------------------------------------------
 * mtr_call_alleles_device splits a locus' reads by one integer, so two alleles of one length - (CAG)20 against (CAG)10(CAA)10, a pure CGG tract
 * against one with AGG interruptions - are one allele to it, and the consensus votes them into a mixture.  This call splits by SEQUENCE: the
 * edit distance between every two supporting reads' oriented windows, and an exact one- or two-medoid split over those distances.  The
 * reference has nothing of this kind; the definition is this project's own.
 * Input is mtr_consensus_src as mtr_allele_consensus_device takes it: the joined rows ascending by (read, locus), their windows, and
 * support_off and read of a mtr_call_alleles_device result over the same rows - membership and min_ratio are decided there, the list order is
 * ascending (value, read).  allele and zygosity of the src are not read and may be NULL.  value [n_support] (int32, DEVICE) holds the calls'
 * values; it is carried along and never compared.  Parameters mtr_seq_params { max_dist K, min_support, min_percent, min_sep, min_gain }.
 * The definition:
 *   members     the members of locus l are its S_l entries in list order, t = 0 .. S_l - 1; each finds its row by bisection over (read, locus)
 *               as in the consensus; W_t is its oriented window, n_t its length
 *   distance    D(t, u) = min(lev(W_t, W_u), K + 1), lev the unit-cost edit distance: symmetric, D(t, t) = 0.  K in 0 .. MTR_SEQ_MAX_DIST = 254,
 *               so a distance fits one byte.  By definition D = K + 1 when |n_t - n_u| > K, and when either window exceeds
 *               MTR_CONS_MAX_WINDOW.  The definition does not depend on how it is computed: the kernels fill the band of diagonals
 *               ba_band(n, m, (K - |m - n|) >> 1), at most K + 1 wide; a path of cost <= K cannot leave it, so the banded result clamped to
 *               K + 1 is exactly D - unlike the consensus' band, which is part of its definition, this band is only the way there
 *   skipped     a locus with S_l > MTR_SEQ_MAX_MEMBERS = 128: skipped[l] = 1, no pairs are computed, the entries keep list order and allele 0,
 *               zygosity 0, call, call_support and cost zeros, medoid (-1, -1)
 *   one medoid  cost(c) = sum over u of D(c, u); c* = the smallest c of least cost, cost1 = cost(c*)
 *   two medoids for every pair c0 < c1: member u belongs to c0 iff D(c0, u) <= D(c1, u) (ties go to c0), else to c1; n0, n1 the two sizes;
 *               cost2(c0, c1) = sum over u of min(D(c0, u), D(c1, u))
 *   admissible  a pair is admissible iff min(n0, n1) >= min_support, min(n0, n1) * 100 >= min_percent * S_l (in int64), D(c0, c1) >= min_sep,
 *               and cost2 * 100 <= cost1 * (100 - min_gain) (in int64)
 *   S_l < min_support (S_l == 0 too)   zygosity 0, medoid (-1, -1), call, call_support and cost zeros; the entries keep list order, allele 0
 *   no admissible pair                 zygosity 1, medoid (read of c*, -1), call (value[c*], value[c*]), call_support (S_l, 0), cost (cost1,
 *                                      cost1); the entries keep list order, allele 0
 *   an admissible pair exists          zygosity 2: the admissible pair of smallest cost2, ties to the smallest c0, then the smallest c1; medoid the
 *                                      two reads, call their values, call_support (n0, n1), cost (cost1, cost2); the entries are the STABLE
 *                                      PARTITION of the list - allele 0's members in list order, then allele 1's: the 0 .. 0 1 .. 1 column the
 *                                      consensus requires
 * Every output is an exact integer and none depends on the order in which the device worked.  Columns: support_off [n_loci + 1], a copy; value,
 * read, allele, dist_to_medoid [S] each - the distance to the entry's own medoid, 0 under zygosity 0; zygosity [n_loci]; call, call_support,
 * medoid [n_loci * 2] each; cost [n_loci * 2] int64; skipped [n_loci]; pair_off [n_loci + 1] int64 - locus l owns S_l (S_l - 1) / 2 pairs, none
 * when skipped; dist [P] uint8, the upper triangle of D row-major: pair (t < u) at pair_off[l] + t * S_l - t (t + 1) / 2 + (u - t - 1).  The
 * first eight are mtr_allele_calls_dst's columns: mtr_allele_consensus_device takes them as it takes mtr_call_alleles_device's.
 *
 * mtr_call_alleles_sequence_device computes into buffers of the context's own and keeps them (compute, then copy, as mtr_window_edits_device);
 * it needs no uploaded batch and touches nothing that a batch, a run or another call keeps.  *out_support = S, *out_pairs = P.  Checked in this
 * order, each MTR_ERR_BAD_ARG naming the offender: NULL ctx, out_support or out_pairs; NULL src or prm; n_loci < 1 or above 2^30 - 1, n_rows,
 * n_support or n_bases outside 0..2^31 - 1; max_dist (0 .. MTR_SEQ_MAX_DIST), min_support (>= 1), min_percent (0..50), min_sep (>= 1), min_gain
 * (0..100), in this order; a NULL input column that would be read (value among them); an input column that is not device memory of the
 * context's GPU or runs past its allocation; then on the device the rows' order, the offset columns (ascending from 0 to n_bases /
 * n_support, no window above 2^30 bases), an entry without a row.  More than 2^31 - 1 pairs are MTR_ERR_OVERFLOW.  wait_stream is the stream
 * that wrote the columns, handled as mtr_upload_batch_device handles it.  mtr_call_alleles_sequence_copy_device copies what the last successful
 * call kept, device to device, into caller-owned DEVICE memory: MTR_ERR_BAD_ARG without such a call or with a NULL dst or column that would be
 * written (value, read, allele and dist_to_medoid may be NULL only when S == 0, dist only when P == 0); cap_loci < n_loci, cap_support < S or
 * cap_pairs < P: MTR_ERR_OVERFLOW; a failure writes nothing.  The context's stream is synchronised before either returns.  MTR_ABI_VERSION is
 * unchanged by these entries: look for them by symbol. */
#define MTR_SEQ_MAX_DIST 254
#define MTR_SEQ_MAX_MEMBERS 128
typedef struct mtr_seq_params {
    int32_t max_dist;      /* K: distances saturate at K + 1 */
    int32_t min_support;   /* the fewest reads an allele needs */
    int32_t min_percent;   /* the smaller allele's least share of the locus' supporting reads, in percent */
    int32_t min_sep;       /* the least distance between the two medoids */
    int32_t min_gain;      /* the least saving of cost2 against cost1, in percent */
} mtr_seq_params;
typedef struct mtr_seq_calls_dst {
    int64_t *support_off;     /* [n_loci + 1] */
    int32_t *value;           /* [S] */
    int32_t *read;            /* [S] */
    uint8_t *allele;          /* [S] */
    uint8_t *zygosity;        /* [n_loci] */
    int32_t *call;            /* [n_loci * 2] */
    int32_t *call_support;    /* [n_loci * 2] */
    int64_t *cost;            /* [n_loci * 2] cost1, cost2 */
    int32_t *medoid;          /* [n_loci * 2] the medoids' reads, -1 without one */
    int32_t *dist_to_medoid;  /* [S] */
    uint8_t *skipped;         /* [n_loci] */
    int64_t *pair_off;        /* [n_loci + 1] */
    uint8_t *dist;            /* [P] */
    int64_t  cap_loci;
    int64_t  cap_support;
    int64_t  cap_pairs;
} mtr_seq_calls_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_call_alleles_sequence_device(mtr_ctx *ctx, const mtr_consensus_src *src, const int32_t *value, const mtr_seq_params *prm,
                                            void *wait_stream, int64_t *out_support, int64_t *out_pairs);
mtr_status mtr_call_alleles_sequence_copy_device(mtr_ctx *ctx, const mtr_seq_calls_dst *dst);

/* ---- genotype quality: each read scored against both allele sequences, the scores reduced to genotype likelihoods ------------------------------
 * The calls say "two alleles, these"; the consensus says what they are.  This call says how sure that is: per read how much better it fits one
 * allele's sequence than the other's, per locus the likelihoods of the genotypes 0/0, 0/1 and 1/1 on the Phred scale (a VCF's PL and GQ).  The
 * reference has nothing of this kind; the definition is this project's own.  Every output is an exact integer and none depends on the order in
 * which the device worked.
 * Input, all DEVICE memory: mtr_consensus_src exactly as mtr_allele_consensus_device takes it - rows ascending by (read, locus), windows,
 * support_off, read, allele, zygosity; win_qual [n_bases] aligned with win_bases, NULL meaning that every quality is qual_cap; the alleles'
 * sequences cons_off [2 * n_loci + 1], cons_bases [n_cons] with the allele index A = 2 * locus + a, as the consensus writes them.  Parameters
 * mtr_gq_params { band_extra 0..MTR_CONS_MAX_EXTRA, qual_cap 1..MTR_CONSQ_MAX_CAP, gap_cap 1..qual_cap, read_cap 1..MTR_GQ_MAX_READ_CAP = 2^20 }.
 * The definition:
 *   alleles     allele a of locus l exists iff zygosity[l] > a.  The spans of alleles that do not exist are not read
 *   weights     omega[i] = min(max(q_i, 1), qual_cap) for the base of quality q_i; gamma(i), 0 <= i <= n, the gap weight of the quality-weighted
 *               consensus: the lighter of the two bases beside boundary i, the one that exists at the ends, 1 for an empty window
 *   score       s(e, a) of support entry e (window W of n bases, found by bisection over (read, locus) as in the consensus) against existing
 *               allele a (sequence C of m bases): over the consensus' band - cells (i, j) exist iff dlo <= j - i <= dhi, dlo = min(0, m - n) -
 *               band_extra, dhi = max(0, m - n) + band_extra; the band is part of the definition - D(0, 0) = 0, else D(i, j) is the minimum of
 *               diag = D(i-1, j-1) + (W[i-1] != C[j-1] ? omega[i-1] : 0), up = D(i-1, j) + min(omega[i-1], gap_cap), left = D(i, j-1) +
 *               min(gamma(i), gap_cap).  s = D(n, m), an int32: at most 32 768 steps of at most 93
 *   scored      an entry is scored iff for every existing allele of its locus the consensus' skip rule (n or m above MTR_CONS_MAX_WINDOW, or
 *               |m - n| + 2 * band_extra + 1 > MTR_CONS_MAX_BAND) is false.  An entry that is not scored has s = -1 against both alleles and
 *               takes no part in any sum.  A locus of zygosity 0 scores nothing
 *   per entry   score [S, 2] int32, -1 where there is none.  Zygosity 2 and scored: best [S] uint8 is 0 if s0 < s1, 1 if s1 < s0, the entry's own
 *               allele on a tie; margin [S] int32 is |s0 - s1|.  Zygosity 1 and scored: best = 0, margin = 0.  Otherwise best is the entry's
 *               allele, margin = 0
 *   per locus   c(x) = min(x, read_cap), x0 = c(s0), x1 = c(s1); T = {3, 3, 2, 2, 1, 1, 1, 1, 1, 1}, T[d] = 0 for d >= 10 - 10 log10(1 +
 *               10^(-d/10)) rounded, the integer form of a read drawn from either allele with probability one half; h = min(x0, x1) + 3 -
 *               T[min(|x0 - x1|, 10)].  Zygosity 2: raw [n_loci, 3] int64 is the sum over the scored entries of (x0, h, x1), for the genotypes
 *               0/0, 0/1 and 1/1; pl [n_loci, 3] int64 = raw - min(raw); gt [n_loci] uint8 is the genotype of least raw (0, 1, 2 in that
 *               order of genotypes), ties in the order 0/1, 0/0, 1/1; gq [n_loci] int64 is the least pl among the other two.  Zygosity 1: raw =
 *               (sum of x0, -1, -1), pl = (0, -1, -1), gt = 0, gq = -1.  Zygosity 0: raw and pl all -1, gt = 255, gq = -1.  scored and
 *               unscored [n_loci] int32 count the locus' entries either way (both 0 under zygosity 0)
 * With qual_cap = gap_cap = 1 every s is the consensus' unit-cost banded distance D(n, m), whatever the qualities.  With one constant quality c <=
 * gap_cap and no empty window every s is c times that.
 * All sizes follow from the input: one call, no size call.  Checked in this order, each MTR_ERR_BAD_ARG naming the offender: NULL ctx; NULL src,
 * prm or dst; n_loci < 1 or above 2^30 - 1, n_rows, n_support, n_bases or n_cons outside 0..2^31 - 1; band_extra, qual_cap, gap_cap, read_cap in
 * this order; a NULL input column that would be read (cons_off always, cons_bases with n_cons > 0; win_qual may be NULL); an input column that is
 * not device memory of the context's GPU or runs past its allocation; then on the device the rows' order, the offset columns, a zygosity above
 * 2, an entry without a row, an allele column that is not 0 .. 0 1 .. 1 within a locus, a cons_off that does not ascend from 0 to n_cons (the
 * smallest such allele index is named).  Then cap_support < n_support or cap_loci < n_loci: MTR_ERR_OVERFLOW; a NULL destination column (score,
 * best and margin may be NULL only when n_support == 0), or one that is not device memory: MTR_ERR_BAD_ARG.  A failed call writes nothing.  The
 * context's stream is synchronised before the call returns; wait_stream is the stream that wrote the columns, handled as
 * mtr_upload_batch_device handles it.  The call needs no upload and touches nothing that a batch, a run or another call keeps.
 * MTR_ABI_VERSION is unchanged by this entry: look for it by symbol. */
#define MTR_GQ_MAX_READ_CAP (1 << 20)
typedef struct mtr_gq_params {
    int32_t band_extra;    /* the consensus' band */
    int32_t qual_cap;      /* where a base's weight saturates */
    int32_t gap_cap;       /* where a gap step's cost saturates */
    int32_t read_cap;      /* where one read's score saturates in the locus' sums */
} mtr_gq_params;
typedef struct mtr_gq_dst {
    int32_t *score;       /* [S * 2] */
    uint8_t *best;        /* [S] */
    int32_t *margin;      /* [S] */
    int64_t *raw;         /* [n_loci * 3] */
    int64_t *pl;          /* [n_loci * 3] */
    uint8_t *gt;          /* [n_loci] */
    int64_t *gq;          /* [n_loci] */
    int32_t *scored;      /* [n_loci] */
    int32_t *unscored;    /* [n_loci] */
    int64_t  cap_support;
    int64_t  cap_loci;
} mtr_gq_dst;   /* caller-owned DEVICE memory */
mtr_status mtr_genotype_quality_device(mtr_ctx *ctx, const mtr_consensus_src *src, const uint8_t *win_qual, const int64_t *cons_off, const uint8_t *cons_bases,
                                       int64_t n_cons, const mtr_gq_params *prm, void *wait_stream, const mtr_gq_dst *dst);

/* ---- several GPUs in ONE process: the one exchange of the path (ABI 5) --------------------------------------------------
 * Reads shard over the GPUs of a node (isolated semantics make every read an independent unit); what is left
 * of handle_one_file.c:281-287's loop across GPUs is ONE exchange: the record tables travel to the process that chains and
 * prints (chaining.cpp).  A mtr_gather owns an RCCL communicator per GPU (ncclCommInitAll: one process, N devices) and
 * moves the wire form device to device over xGMI to the first GPU, from there in one copy to pinned host memory:
 *   mtr_gather_stage     a GPU's finished batch (after mtr_wait) is compacted to the wire form into a staging buffer on ITS OWN
 *                        device; returns a ticket.  Thread-safe: every GPU's host thread calls it for its own batches.
 *   mtr_gather_exchange  the staged tables named by tickets[0..n) - any number per GPU - go to the first GPU:
 *                        ncclGroupStart; per ticket ncclSend on the owner's communicator + ncclRecv on the first GPU's;
 *                        ncclGroupEnd; then ONE device-to-host copy.  out_ptrs[i] / out_bytes[i] = ticket i's table in pinned
 *                        host memory owned by the gather, valid until the next exchange; the tickets are released.  One
 *                        caller at a time.  Tables of the first GPU itself skip the collective (MTR_GATHER_SELF=1 sends
 *                        them through ncclSend/ncclRecv to itself as well: the RCCL path on a one-GPU box).
 * librccl.so is bound at run time by mtr_gather_create and only there, so a single-GPU process never loads it; RCCL needs
 * devices[] distinct (it takes a device once per communicator) - a gather over repeated devices works through the host copies. */
typedef struct mtr_gather mtr_gather;
mtr_status mtr_device_count(int32_t *out_count);
mtr_status mtr_gather_create(int32_t n_ranks, const int32_t *devices, mtr_gather **out);
void       mtr_gather_destroy(mtr_gather *g);
const char *mtr_gather_last_error(const mtr_gather *g);
mtr_status mtr_gather_stage(mtr_gather *g, int32_t rank, mtr_ctx *ctx, int32_t *counts_host, int64_t *out_total_records,
                            int64_t *out_bytes, int32_t *out_ticket);
mtr_status mtr_gather_exchange(mtr_gather *g, int32_t n_tickets, const int32_t *tickets, const uint8_t **out_ptrs, int64_t *out_bytes);
/* RCCL comes up in the background (loading librccl.so + ncclCommInitAll: ~2 s on an MI355X box, more than a 100 000-read job takes): mtr_gather_create
 * returns at once, and an exchange that finds RCCL not up yet - or not usable: librccl missing, a device given twice - copies its tables from every GPU's
 * staging buffer straight into the pinned host buffer instead; the results are the same.  mtr_gather_wait_ready blocks until RCCL is up (MTR_OK) or known
 * to be unusable (MTR_ERR_NO_DEVICE, reason in mtr_gather_last_error).  mtr_gather_get_stats: out[0] exchanges over RCCL, [1] exchanges straight to the host,
 * [2] / [3] their bytes, [4] ms RCCL took to come up, [5] 1 = up, 0 = still coming up, -1 = not usable.  mtr_gather_destroy does not wait for a library
 * that is still coming up: it leaves the object to the process's end, and such a process should leave through _exit. */
mtr_status mtr_gather_wait_ready(mtr_gather *g);
mtr_status mtr_gather_get_stats(const mtr_gather *g, int64_t *out, int32_t n);

/* File-order mode = the reference's own behaviour on a multi-read file (leak A, and H2) instead of
 * isolated semantics.  The reference's inputString_w_rand and orgInputString live for the whole file
 * (handle_one_file.c:85, mTR.h:65-67): the window look-ahead of a read (fill_directional_index.c:232) and the one-past
 * reads of its DPs (wrap_around_DP.c:243-245) see what the most recent LONGER read left beyond the part the current
 * read rewrites.  A mtr_file_state is the shadow of that state for ONE file; give it the batches of the file in
 * file order (any context, any batch size — the state carries over) through mtr_upload_batch_in_file instead of
 * mtr_upload_batch, then run / fetch as usual.  Results then equal the reference run on the whole file at the lower
 * edge (the arguments of insert_an_alignment_into_set, read after read); the printed chain can still differ where two
 * chains tie, because the reference breaks those ties by heap address (chaining.cpp:201).  Reads no longer read
 * preceded take the normal path; the others run their range phase with plain 1024-bin window histograms (slower).
 * Shards of a file given to different GPUs need the state of the reads before the shard: feed those lengths/bases
 * through mtr_file_state_skip. */
typedef struct mtr_file_state mtr_file_state;
mtr_status mtr_file_state_create(mtr_file_state **out);
void       mtr_file_state_destroy(mtr_file_state *fs);
mtr_status mtr_upload_batch_in_file(mtr_ctx *ctx, mtr_file_state *fs, const uint8_t *bases, const int64_t *offsets,
                                    const int32_t *lens, int32_t n_reads);
/* advance the state over reads that another context / GPU processes (same arguments as an upload, no device work) */
mtr_status mtr_file_state_skip(mtr_file_state *fs, const uint8_t *bases, const int64_t *offsets, const int32_t *lens, int32_t n_reads);

/* File-order mode for reads that are already in DEVICE memory: the same state fed from the device.  The arguments, the checks and
 * the stream protocol are those of mtr_upload_batch_device / mtr_upload_fasta_device; fs == NULL is MTR_ERR_BAD_ARG.  The stale
 * tails and the two bases after each read are made by kernels (mtr_amd/csrc/file_order.hip.inc) from the packed words of the reads
 * that left them; the results equal those of mtr_upload_batch_in_file on the same reads, and no base crosses to the host.
 * A state fed this way keeps the lengths of its stairs on the host and their 2-bit words in device memory that it owns, on the
 * GPU of the first context that fed it (mtr_file_state_destroy frees it there).  A state is host-fed or device-fed, fixed by its
 * first feed: the other kind of call on it, or a context on another GPU, is MTR_ERR_BAD_ARG with the reason in mtr_last_error
 * (mtr_file_state_skip has no context: the status alone).  A refused upload - a byte that is no base, a bad argument, a FASTA read
 * longer than MTR_MAX_READ_LENGTH - leaves no batch uploaded and the state exactly as it was.  A FASTA stop uploads the reads before
 * it and the state advances over those; no reads: no batch, the state unchanged.
 * mtr_file_state_skip_device advances the state over reads in device memory that another GPU processes: they are packed and checked
 * into the state's storage; no batch is uploaded and the context's resident batch stays as it is.  n_reads == 0 is MTR_OK. */
mtr_status mtr_upload_batch_device_in_file(mtr_ctx *ctx, mtr_file_state *fs, const uint8_t *d_text, int64_t text_bytes, const int64_t *offsets,
                                           const int32_t *lens, int32_t n_reads, int32_t text_kind, void *wait_stream);
mtr_status mtr_upload_fasta_device_in_file(mtr_ctx *ctx, mtr_file_state *fs, const uint8_t *d_fasta, int64_t n_bytes, void *wait_stream,
                                           mtr_fasta_info *info);
/* a FASTQ file's reads as the next reads of the file: feeds and advances a device-fed state exactly as mtr_upload_fasta_device_in_file */
mtr_status mtr_upload_fastq_device_in_file(mtr_ctx *ctx, mtr_file_state *fs, const uint8_t *d_fastq, int64_t n_bytes, void *wait_stream,
                                           mtr_fasta_info *info);
mtr_status mtr_file_state_skip_device(mtr_ctx *ctx, mtr_file_state *fs, const uint8_t *d_text, int64_t text_bytes, const int64_t *offsets,
                                      const int32_t *lens, int32_t n_reads, int32_t text_kind, void *wait_stream);

/* ---- a FASTA or FASTQ file in device memory, batch by batch ----------------------------------------------------------------
 * The entry points above make ONE batch of the whole buffer.  A caller who wants batches of a chosen size cannot cut the file
 * by looking at it: a FASTA record ends where the next header window - an fgets window of 4095 bytes that starts with '>' - begins, which
 * is a result of the parse and not of a search for "\n>".  The _window entry points take the FIRST n_bytes of a longer input:
 *   more_follows == 0  the buffer is the whole (rest of the) input: exactly the entry point of the same kind without _window -
 *                      same code path, same results
 *   more_follows == 1  bytes follow behind the buffer, and nothing is known about them
 *   any other value    MTR_ERR_BAD_ARG
 * fs == NULL is isolated mode (mtr_upload_fasta_device); otherwise file-order mode (mtr_upload_fasta_device_in_file): the state
 * advances over the uploaded reads only.  Protocol, argument checks, stream handling and mtr_fasta_index are those of the entry
 * points above.  With more_follows == 1:
 *   a stop     found in the window is a stop of the whole input: line starts, fgets windows, hidden bytes, base counts and header
 *              windows are functions of the bytes before a position.  It is reported as ever, with the reads closed before it.
 *              Not raised are the two FASTQ stops that only the end of the input or a complete line decides: "the file ends
 *              inside a record", and the length of a quality line whose LF is not in the window
 *   FASTA      without a stop: the reads are the records closed by a header window that begins inside the window.  The last
 *              record is open and is not returned.  end = MTR_FASTA_END_MORE, end_pos = the position of the open record's header
 *              '>' - or 0 if the open record is the window's first, because that record owns the bases in front of its header too;
 *              no header window at all: no reads, end_pos 0.  A header window starts an fgets window, so a parse that begins at
 *              end_pos puts every later window where the parse of the whole input puts it: resuming there is exact
 *   FASTQ      without a stop: the reads are the records whose quality line's LF lies inside the window.  end =
 *              MTR_FASTA_END_MORE, end_pos = the byte behind the last such LF: the open record's header line, or n_bytes if the
 *              window ends exactly behind a record
 *   n_bytes == 0   MTR_OK, no reads, MTR_FASTA_END_MORE, end_pos 0
 *   n_reads == 0 with MTR_FASTA_END_MORE   the window is smaller than its first record: the caller widens it
 *   info.n_bases, id_bytes, the compaction, the IDs, and mtr_upload_fastq_device's packing out of the file itself cover the
 *   returned reads only.  The parser's buffers in the context are sized by n_bytes, so a walk keeps them at window size.
 * The walk of an input of any length - only a window is limited to INT32_MAX bytes:
 *   pos = 0;
 *   do { n = min(w, len - pos);
 *        mtr_upload_fasta_device_window(ctx, fs, d + pos, n, pos + n < len, stream, &info);
 *        if (info.end == MTR_FASTA_END_MORE && info.n_reads == 0) { w *= 2; continue; }
 *        if (info.n_reads > 0) { run; report; }            // info.end_pos + pos is the position in the input
 *        pos += info.end_pos;
 *   } while (info.end == MTR_FASTA_END_MORE);
 * The reads of all batches together, and the last call's end, bad_char and pos + end_pos, are those of one call on the whole
 * input, whatever the windows. */
#define MTR_FASTA_END_MORE 5
mtr_status mtr_parse_fasta_device_window(mtr_ctx *ctx, const uint8_t *d_fasta, int64_t n_bytes, int32_t more_follows,
                                         void *wait_stream, const mtr_fasta_dst *dst, mtr_fasta_info *info);
mtr_status mtr_upload_fasta_device_window(mtr_ctx *ctx, mtr_file_state *fs, const uint8_t *d_fasta, int64_t n_bytes,
                                          int32_t more_follows, void *wait_stream, mtr_fasta_info *info);
mtr_status mtr_parse_fastq_device_window(mtr_ctx *ctx, const uint8_t *d_fastq, int64_t n_bytes, int32_t more_follows,
                                         void *wait_stream, const mtr_fasta_dst *dst, mtr_fasta_info *info);
mtr_status mtr_upload_fastq_device_window(mtr_ctx *ctx, mtr_file_state *fs, const uint8_t *d_fastq, int64_t n_bytes,
                                          int32_t more_follows, void *wait_stream, mtr_fasta_info *info);

/* orgInputString[L] and [L+1] as read i of the resident batch found them: 0 under isolated semantics, in file-order mode
 * the bases an earlier, longer read left there.  A repeat can end on them (wrap_around_DP.c:243-245), and a printer of
 * the -a alignments (mtr_alignments) needs them for its top row. */
mtr_status mtr_get_bases_after_read(const mtr_ctx *ctx, int32_t read_idx, uint8_t out[2]);

/* The -a alignments (replaces pretty_print_alignment, wrap_around_DP.c:57-213, for the repeats the caller chose to
 * report, i.e. after chaining): for n records of reads of the RESIDENT batch (mtr_process_batch / mtr_upload_batch
 * leaves it on the device) the wrap-around alignment of org[rep_start .. rep_end] against the record's unit with the
 * record's own (match_gain, mismatch_penalty, indel_penalty).  Result: one byte per alignment column in TRACEBACK order
 * (last column first, as the reference builds its three rows): 1 = match, 2 = mismatch, 3 = gap in the read
 * (deletion), 4 = gap in the unit (insertion).  (*out_off)[i] .. (*out_off)[i+1] is record i's slice of *out_ops;
 * (*out_end)[2i] is the 0-origin read position of the last aligned base and (*out_end)[2i+1] the 1-origin unit
 * column it is aligned to (where the walk back through the columns starts).  The three arrays are malloc'ed;
 * free() them. */
mtr_status mtr_alignments(mtr_ctx *ctx, int32_t n, const int32_t *read_idx, const mtr_record *records,
                          uint8_t **out_ops, int64_t **out_off, int32_t **out_end);

/* Device time of the last mtr_run_resident()/mtr_process_batch(), measured with HIP events on the stream the kernels were
 * launched on.  Ids: 0 = the range kernel when it runs alone (test entry points), 1 = the whole launch; and the phases of the
 * staged chain (launches = 0 for a batch the per-read kernel ran): 2 = candidate ranges, 3 = unit search (k-mer tables, seeds, walks),
 * 4 = two-parameter alignments, 5 = selection, 6 = revisions, 7 = comparison over k + replay of the sequential range loop. */
#define MTR_N_KERNEL_TIMES 10   /* 8, 9 (ABI 5): the two dominant kernels of the chain by themselves, launches of both passes summed -
                                 * 8 = mtr_k_revise_quads (four revisions per wavefront), 9 = mtr_k_dp2_quads (four alignments per wavefront);
                                 * launches = 0 when the batch ran one DP per wavefront (small batches) or in the per-read kernel */
typedef struct mtr_kernel_time { float ms; int32_t launches; } mtr_kernel_time;
mtr_status mtr_get_kernel_times(const mtr_ctx *ctx, mtr_kernel_time *out, int32_t n_kernels);

/* Work counters of the last run, accumulated on the device (used for the roofline figures):
 * [0] wrap-around DP calls, [1] DP cells, [2] DP rows, [3] revision DP calls, [4] revision DP cells,
 * [5] k-mer tables built, [6] k-mer look-ups, [7] candidate ranges, [8] ranges executed, [9] records,
 * [10] DI passes, [11] DI positions, [12] traceback steps, [13] undefined-behaviour guards hit. */
#define MTR_N_COUNTERS 56   /* [16..31]: shader-clock cycles per phase summed over wavefronts (total, DP forward, DP
                             * traceback, table build, seed list, walks, polish, revision votes, slot copies,
                             * revision DP forward / traceback, range-finder phases);
                             * [32] wrap_around_DP calls answered from the per-range memo (same window, same unit),
                             * [33] DP cells those calls would have filled, [34] k-mer tables proven unnecessary;
                             * [48..51] four-per-wavefront passes: cell bytes written / cells of the DPs served, alignments then revisions;
                             * [52] revisions answered by an identical revision of the same range, [53] reads the chain sent back to the per-read kernel,
                             * [54] candidate ranges the chain searched ([8]: the ranges the reference's loop reaches) */
mtr_status mtr_get_counters(const mtr_ctx *ctx, int64_t *out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* MTR_HIP_H */
