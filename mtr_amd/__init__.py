"""mtr_amd — MI355X (gfx950) implementation of reference mTR's per-read hot path.

Python host-side mirror of the C-ABI in include/mtr_hip.h (ctypes; plain pointers).  Only the device-input and report methods
(Engine.upload_device / process_device / parse_fasta_device / upload_fasta_device / parse_fastq_device / upload_fastq_device /
walk_fasta_device / walk_fastq_device /
export_tensor / report_tensors / report_alignment_tensors / report_text / report_bytes / report_motif_tensors / search_motifs / search_motif_loci /
search_flanks / genotype_loci / genotype_catalog / genotype_partial / genotype_partial_catalog) take or return torch tensors;
they import torch when called.
The product path is libmtr_hip.so only: importing works without a GPU, but creating an Engine
without the library or without a HIP device raises — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, NamedTuple, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTR_LIB", os.path.join(HERE, "libmtr_hip.so"))   # MTR_LIB: A/B another build of the library
MAX_PERIOD = 500
MAX_READ_LENGTH = 833333                     # MTR_MAX_READ_LENGTH
TEXT_ASCII, TEXT_CODES = 0, 1                # MTR_TEXT_ASCII, MTR_TEXT_CODES
FASTA_TILE_BYTES = 4096                      # MTR_FASTA_TILE_BYTES (mtr_amd/csrc/fasta.hip.inc): the bytes of a FASTA file one workgroup scans
FASTA_END = {0: "eof", 1: "empty", 2: "bad", 3: "toolong"}        # MTR_FASTA_END_* of a FASTA file
FASTQ_END = {**FASTA_END, 4: "format", 5: "more"}        # ... of a FASTQ file: MTR_FASTA_END_FORMAT too; of a window: MTR_FASTA_END_MORE

STATUS = {0: "MTR_OK", 1: "MTR_ERR_NO_DEVICE", 2: "MTR_ERR_BAD_ARG", 3: "MTR_ERR_OOM", 4: "MTR_ERR_HIP",
          5: "MTR_ERR_OVERFLOW", 6: "MTR_ERR_DP_TOO_LARGE"}
COUNTER_NAMES = ["dp_calls", "dp_cells", "dp_rows", "revise_dp_calls", "revise_dp_cells", "kmer_tables", "kmer_lookups",
                 "ranges_candidate", "ranges_executed", "records", "di_passes", "di_positions", "traceback_steps",
                 "undefined_guards", "global_tables", "reserved",
                 "cyc_total", "cyc_dp_fwd", "cyc_dp_tb", "cyc_tab_build", "cyc_seeds", "cyc_walk", "cyc_polish", "cyc_revise_vote",
                 "cyc_slot_copy", "cyc_dp_fwd_rev", "cyc_dp_tb_rev", "cyc_k1_codes", "cyc_k1_passes", "cyc_k1_extract",
                 "cyc_k1_dedup", "cyc_k1_total",
                 "memo_hits", "memo_cells", "tables_skipped", "cyc_tb_refill", "tb_refills", "walk_steps", "walk_slow_steps", "cyc_walk_slow",
                 "walk_calls", "walk_closed", "cyc_walk_fast", "prof43", "prof44", "prof45", "prof46", "prof47",
                 "qpass_bytes_dp2", "qpass_cells_dp2", "qpass_bytes_rev", "qpass_cells_rev", "revisions_shared", "reads_sent_back", "ranges_searched", "prof55"]
# prof43..47, prof55: scratch counters of the profiling builds (-DMTR_PROFILE...); what they count depends on the kernel that wrote them
# (per-read kernel: revisions / unchanged units / accepted rounds; walk kernels: cycles by window width; see the CNT_SPARE* uses in csrc).
# In a product build (no -DMTR_PROFILE) mtr_k_dp2_quads counts its passes by kind: prof47 = four alignments per wavefront, prof55 = eight
EXPORTS = ["mtr_create", "mtr_destroy", "mtr_last_error", "mtr_abi_version", "mtr_process_batch", "mtr_free_results",
           "mtr_upload_batch", "mtr_run_resident", "mtr_fetch_results", "mtr_get_kernel_times", "mtr_get_counters",
           "mtr_test_ranges", "mtr_test_ranges_parts", "mtr_test_wrap_dp", "mtr_test_wrap_dp_pass", "mtr_test_polish", "mtr_test_revise", "mtr_test_last_mode", "mtr_set_trace", "mtr_get_trace",
           "mtr_run_resident_async", "mtr_wait", "mtr_alignments",
           "mtr_file_state_create", "mtr_file_state_destroy", "mtr_upload_batch_in_file", "mtr_file_state_skip",
           "mtr_get_bases_after_read", "mtr_upload_batch_packed", "mtr_fetch_results_packed", "mtr_export_packed_device",
           "mtr_unpack_records", "mtr_pack_records", "mtr_get_first_failed_read", "mtr_upload_batch_device",
           "mtr_report_device", "mtr_test_chain", "mtr_report_alignments_device", "mtr_report_text_device", "mtr_test_report_lines",
           "mtr_parse_fasta_device", "mtr_upload_fasta_device", "mtr_fasta_index",
           "mtr_parse_fastq_device", "mtr_upload_fastq_device", "mtr_upload_fastq_device_in_file",
           "mtr_upload_batch_device_in_file", "mtr_upload_fasta_device_in_file", "mtr_file_state_skip_device", "mtr_test_file_tail",
           "mtr_parse_fasta_device_window", "mtr_upload_fasta_device_window", "mtr_parse_fastq_device_window", "mtr_upload_fastq_device_window",
           "mtr_report_motifs_device", "mtr_test_unit_motifs", "mtr_search_motifs_device",
           "mtr_search_motif_loci_device", "mtr_motif_loci_copy_device", "mtr_search_flanks_device", "mtr_genotype_loci_device",
           "mtr_call_alleles_device", "mtr_genotype_partial_device", "mtr_genotype_catalog_device", "mtr_genotype_catalog_copy_device",
           "mtr_call_alleles_rows_device", "mtr_test_catalog_stats", "mtr_genotype_partial_catalog_device", "mtr_genotype_partial_catalog_copy_device",
           "mtr_test_partial_catalog_stats", "mtr_catalog_create", "mtr_catalog_destroy", "mtr_catalog_info_get", "mtr_genotype_catalog_prepared_device",
           "mtr_genotype_partial_catalog_prepared_device", "mtr_test_catalog_dump", "mtr_test_catalog_build_stats",
           "mtr_extract_windows_device", "mtr_allele_consensus_device", "mtr_window_structure_device",
           "mtr_window_edits_device", "mtr_window_edits_copy_device", "mtr_test_window_edits_rounds",
           "mtr_call_alleles_sequence_device", "mtr_call_alleles_sequence_copy_device",
           "mtr_keep_qualities", "mtr_attach_qualities_device", "mtr_qualities_resident", "mtr_extract_window_qualities_device",
           "mtr_allele_consensus_quality_device"]
QUAL_MAX, CONSQ_MAX_CAP = 93, 93             # MTR_QUAL_MAX, MTR_CONSQ_MAX_CAP: the largest stored Phred value, the largest qual_cap of Engine.allele_consensus_quality
SEQ_MAX_DIST, SEQ_MAX_MEMBERS = 254, 128     # MTR_SEQ_*: the limits of Engine.call_alleles_by_sequence
WE_FIELDS = 6                               # MTR_WE_FIELDS: pos, segment, copy, column, kind, base of an edit of Engine.window_edits
WS_MAX_SEGMENTS, WS_MAX_WINDOW = 4, 16384    # MTR_WS_*: the limits of Engine.window_structure
CONS_MAX_WINDOW, CONS_MAX_BAND, CONS_INS_SLOTS, CONS_MAX_EXTRA = 16384, 256, 4, 64      # MTR_CONS_*: the limits of Engine.allele_consensus
ALLELE_COPIES, ALLELE_BASES = 0, 1           # MTR_ALLELE_COPIES, MTR_ALLELE_BASES: the measure of Engine.call_alleles
ALIGN_WIDTH = 50                             # MTRH_ALIGN_WIDTH: alignment columns per printed block


class MtrError(RuntimeError):
    pass


class FileState:
    """mtr_file_state: what the reads of ONE file leave behind for the reads after them (file-order mode).  Its first feed fixes
    its kind: host reads (Engine.upload / skip) or reads in device memory (Engine.upload_device / upload_fasta_device /
    skip_device), whose bases it keeps on that GPU."""

    def __init__(self):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.mtr_file_state_create(C.byref(h))
        if st != 0:
            raise MtrError(f"mtr_file_state_create: {STATUS.get(st, st)}")
        self.h = h

    def skip(self, reads):
        bases, offs, lens = _flatten(reads)
        st = self.lib.mtr_file_state_skip(self.h, bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(reads))
        if st != 0:
            raise MtrError(f"mtr_file_state_skip: {STATUS.get(st, st)}")

    def skip_device(self, engine: "Engine", text, offsets, lens, codes: bool = False):
        """mtr_file_state_skip_device: the state advances over reads in device memory (text, offsets, lens, codes as
        Engine.upload_device takes them) that another GPU processes; engine's resident batch is not touched."""
        import torch

        offs, ln = device_input_args(text, offsets, lens, engine.device)
        stream = torch.cuda.current_stream(text.device).cuda_stream
        engine._check(self.lib.mtr_file_state_skip_device(engine.h, self.h, C.c_void_p(text.data_ptr()), text.numel(), offs.ctypes.data, ln.ctypes.data,
                                                          len(ln), TEXT_CODES if codes else TEXT_ASCII, C.c_void_p(stream)), "mtr_file_state_skip_device")

    def close(self):
        if self.h:
            self.lib.mtr_file_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CRecord(C.Structure):
    _fields_ = [("rep_start", C.c_int32), ("rep_end", C.c_int32), ("repeat_len", C.c_int32), ("rep_period", C.c_int32),
                ("num_freq_unit", C.c_int32), ("num_matches", C.c_int32), ("num_mismatches", C.c_int32),
                ("num_insertions", C.c_int32), ("num_deletions", C.c_int32), ("kmer", C.c_int32), ("match_gain", C.c_int32),
                ("mismatch_penalty", C.c_int32), ("indel_penalty", C.c_int32), ("reserved", C.c_int32),
                ("unit", C.c_char * (MAX_PERIOD + 4)), ("unit_score", C.c_int32 * MAX_PERIOD)]


class CReportDst(C.Structure):
    """mtr_report_dst: device pointers of the report's columns and their capacities"""
    _fields_ = [("read", C.c_void_p), ("record", C.c_void_p), ("fields", C.c_void_p), ("ratio", C.c_void_p), ("unit_off", C.c_void_p),
                ("units", C.c_void_p), ("cap_repeats", C.c_int64), ("cap_unit_bytes", C.c_int64)]


class Report(NamedTuple):
    """mTR's report of a batch (Engine.report_tensors): R repeats, the chains of the reads in input order, each in print order.
    counts is on the CPU, every other column on the engine's device."""
    counts: "object"      # int32 [n_reads]: repeats per read
    read: "object"        # int32 [R]
    record: "object"      # int32 [R]: index among the read's records (insertion order, as fetch())
    fields: "object"      # int32 [R, 14]: rep_start .. reserved of mtr_record (0-origin positions)
    ratio: "object"       # float32 [R]: (float)num_matches / repeat_len
    unit_off: "object"    # int64 [R + 1]
    units: "object"       # uint8 [U]: repeat k's unit is units[unit_off[k]:unit_off[k + 1]], ASCII


class CReportAlignDst(C.Structure):
    """mtr_report_align_dst: device pointers of the alignment columns and their capacities"""
    _fields_ = [("col_off", C.c_void_p), ("ops", C.c_void_p), ("text", C.c_void_p), ("first", C.c_void_p),
                ("cap_repeats", C.c_int64), ("cap_columns", C.c_int64)]


class ReportAlignments(NamedTuple):
    """The -a alignments of a Report's repeats (Engine.report_alignment_tensors): C columns in print order, all on the engine's device."""
    col_off: "object"     # int64 [R + 1]: repeat k's columns are col_off[k]:col_off[k + 1]
    ops: "object"         # uint8 [C]: 1 match, 2 mismatch, 3 gap in the read, 4 gap in the unit
    text: "object"        # uint8 [3, C]: the read's bases or '-', '|' or ' ', the unit's bases or '-'
    first: "object"       # int32 [R, 2]: 0-origin read position and 1-origin unit column of the repeat's first column


class CReportTextDst(C.Structure):
    """mtr_report_text_dst: device pointers of the text and the reads' offsets, and the text's capacity"""
    _fields_ = [("text", C.c_void_p), ("read_off", C.c_void_p), ("cap_bytes", C.c_int64)]


class ReportText(NamedTuple):
    """mTR's stdout for a batch (Engine.report_text): B bytes, reads in input order, both tensors on the engine's device."""
    text: "object"        # uint8 [B]
    read_off: "object"    # int64 [n_reads + 1]: read i's bytes are text[read_off[i]:read_off[i + 1]]


class CReportMotifDst(C.Structure):
    """mtr_report_motif_dst: device pointers of the motif catalogue's columns and their capacities"""
    _fields_ = [("strand", C.c_void_p), ("rotation", C.c_void_p), ("motif_len", C.c_void_p), ("group", C.c_void_p),
                ("motif_off", C.c_void_p), ("motifs", C.c_void_p),
                ("g_first", C.c_void_p), ("g_repeats", C.c_void_p), ("g_reads", C.c_void_p), ("g_copies", C.c_void_p), ("g_bases", C.c_void_p),
                ("cap_repeats", C.c_int64), ("cap_groups", C.c_int64), ("cap_motif_bytes", C.c_int64)]


class ReportMotifs(NamedTuple):
    """The motif catalogue of a Report's repeats (Engine.report_motif_tensors): the R repeats' units grouped over rotation and strand
    into G motifs, all on the engine's device.  include/mtr_hip.h defines every column."""
    strand: "object"      # uint8 [R]: 0 = a rotation of the unit is the canonical string, 1 = only one of its reverse complement
    rotation: "object"    # int32 [R]: the smallest such rotation
    motif_len: "object"   # int32 [R]: the primitive period of the unit
    group: "object"       # int32 [R]: the repeat's group
    motif_off: "object"   # int64 [G + 1]
    motifs: "object"      # uint8 [M]: group g's motif is motifs[motif_off[g]:motif_off[g + 1]], ASCII
    g_first: "object"     # int32 [G]: the group's first repeat; groups are numbered in the order of these
    g_repeats: "object"   # int32 [G]: its members
    g_reads: "object"     # int32 [G]: the distinct reads with a member
    g_copies: "object"    # int64 [G]: the sum of num_freq_unit * (unit length / motif_len) over the members
    g_bases: "object"     # int64 [G]: the sum of repeat_len over the members


class CMotifHitsDst(C.Structure):
    """mtr_motif_hits_dst: device pointers of the known-motif search's columns and their capacity"""
    _fields_ = [("fields", C.c_void_p), ("score", C.c_void_p), ("ratio", C.c_void_p), ("strand", C.c_void_p), ("cap_hits", C.c_int64)]


class MotifHits(NamedTuple):
    """What Engine.search_motifs found: one hit per (read, motif) of n reads and m motifs, all on the engine's device.  include/mtr_hip.h
    defines every column."""
    fields: "object"      # int32 [n, m, 8]: start, end (0-origin, inclusive), repeat_len, copies, matches, mismatches, insertions, deletions
    score: "object"       # int32 [n, m]: the best cell's value; 0 = the motif is nowhere in the read (start 0, end -1)
    ratio: "object"       # float32 [n, m]: matches / repeat_len
    strand: "object"      # uint8 [n, m]: 0 = the motif as given, 1 = its reverse complement aligned better


class CMotifLociDst(C.Structure):
    """mtr_motif_loci_dst: device pointers of the locus search's columns and their capacities"""
    _fields_ = [("loci_off", C.c_void_p), ("fields", C.c_void_p), ("score", C.c_void_p), ("ratio", C.c_void_p), ("strand", C.c_void_p),
                ("open", C.c_void_p), ("cap_pairs", C.c_int64), ("cap_loci", C.c_int64)]


class MotifLoci(NamedTuple):
    """What Engine.search_motif_loci found: every locus of every motif in every read, T in all for n reads and m motifs, all on the engine's
    device.  include/mtr_hip.h defines every column."""
    loci_off: "object"    # int64 [n * m + 1]: the loci of (read r, motif k) are rows loci_off[r * m + k] .. loci_off[r * m + k + 1], ascending start
    fields: "object"      # int32 [T, 8]: MotifHits' columns, in read coordinates
    score: "object"       # int32 [T]: at least min_score
    ratio: "object"       # float32 [T]: matches / repeat_len
    strand: "object"      # uint8 [T]
    open: "object"        # uint8 [n, m]: 1 = max_rounds ended the search of this pair with a window left that could still hold a locus


class CFlankHitsDst(C.Structure):
    """mtr_flank_hits_dst: device pointers of the flank search's columns and their capacity"""
    _fields_ = [("dist", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p), ("strand", C.c_void_p), ("cap_hits", C.c_int64)]


class FlankHits(NamedTuple):
    """What Engine.search_flanks found: one hit per (read, pattern) of n reads and m patterns, all on the engine's device.  include/mtr_hip.h
    defines every column."""
    dist: "object"        # int32 [n, m]: the edit distance of the pattern to read[start:end], the smallest over the read
    start: "object"       # int32 [n, m]: 0-origin
    end: "object"         # int32 [n, m]: 0-origin, exclusive
    strand: "object"      # uint8 [n, m]: 0 = the pattern as given, 1 = its reverse complement is nearer


class CGenotypesDst(C.Structure):
    """mtr_genotypes_dst: device pointers of the genotype's columns and their capacity"""
    _fields_ = [("spanning", C.c_void_p), ("orientation", C.c_void_p), ("flank_dist", C.c_void_p), ("window", C.c_void_p), ("fields", C.c_void_p),
                ("score", C.c_void_p), ("ratio", C.c_void_p), ("cap_rows", C.c_int64)]


class Genotypes(NamedTuple):
    """What Engine.genotype_loci found: one row per (read, locus) of n reads and m loci, all on the engine's device.  include/mtr_hip.h defines
    every column.  The allele of a spanning row is window[1] - window[0] bases and fields[3] copies."""
    spanning: "object"    # uint8 [n, m]: 1 = both flanks found in order; 0 = every other column of the row is 0
    orientation: "object" # uint8 [n, m]: 0 = the locus as given, 1 = the read is its reverse complement
    flank_dist: "object"  # int32 [n, m, 2]: the left and the right flank's edit distance
    window: "object"      # int32 [n, m, 2]: the repeat is read[lo:hi]
    fields: "object"      # int32 [n, m, 8]: MotifHits' columns for the window against the motif, in read coordinates
    score: "object"       # int32 [n, m]
    ratio: "object"       # float32 [n, m]: matches / repeat_len

    def to_sparse(self) -> "SparseGenotypes":
        """the spanning rows as Engine.genotype_catalog returns them, sorted by (read, locus): dense results enter the paths that take a
        SparseGenotypes (genotype_windows, join_sparse_genotypes, allele_consensus).  Plain torch (or numpy) over spanning.nonzero()."""
        n, m = int(self.spanning.shape[0]), int(self.spanning.shape[1])
        if hasattr(self.spanning, "detach"):
            import torch

            at = self.spanning.reshape(-1).nonzero().reshape(-1)                 # ascending: row = read * m + locus
            read, locus = torch.div(at, m, rounding_mode="floor").to(torch.int32), (at % m).to(torch.int32)
            cols = [c.reshape((n * m,) + tuple(c.shape[2:]))[at].contiguous() for c in self]
        else:
            at = np.flatnonzero(np.asarray(self.spanning).reshape(-1))
            read, locus = (at // m).astype(np.int32), (at % m).astype(np.int32)
            cols = [np.ascontiguousarray(np.asarray(c).reshape((n * m,) + tuple(np.asarray(c).shape[2:]))[at]) for c in self]
        return SparseGenotypes(n, m, read, locus, *cols, int(len(at)))


class CCatalogDst(C.Structure):
    """mtr_catalog_dst: device pointers of the catalogue genotype's read and locus columns, and the genotype's columns"""
    _fields_ = [("read", C.c_void_p), ("locus", C.c_void_p), ("rows", CGenotypesDst)]


class SparseGenotypes(NamedTuple):
    """What Engine.genotype_catalog found: the R rows of Genotypes with spanning = 1, as a list sorted by (read, locus), all on the engine's
    device.  include/mtr_hip.h defines every column.  Several batches' results are joined with torch.cat per column after the batch's first
    read's index has been added to `read` (and n_reads summed): the joined rows stay sorted."""
    n_reads: int
    n_loci: int
    read: "object"        # int32 [R]
    locus: "object"       # int32 [R]
    spanning: "object"    # uint8 [R]: 1
    orientation: "object" # uint8 [R]
    flank_dist: "object"  # int32 [R, 2]
    window: "object"      # int32 [R, 2]
    fields: "object"      # int32 [R, 8]
    score: "object"       # int32 [R]
    ratio: "object"       # float32 [R]
    candidates: int       # the (read, locus, orientation) candidates the seeds left to be verified

    def to_dense(self) -> "Genotypes":
        """the same rows as Engine.genotype_loci returns them, zeros where a read does not span a locus (n_reads x n_loci rows: small shapes)"""
        import torch

        n, m = self.n_reads, self.n_loci
        at = self.read.long() * m + self.locus.long()
        cols = []
        for c in self[4:11]:
            full = torch.zeros((n * m,) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device)
            full[at] = c
            cols.append(full.reshape((n, m) + tuple(c.shape[1:])))
        return Genotypes(*cols)


class CPartialDst(C.Structure):
    """mtr_partial_dst: device pointers of the partial genotype's columns and their capacity"""
    _fields_ = [("partial", C.c_void_p), ("slot", C.c_void_p), ("flank_dist", C.c_void_p), ("window", C.c_void_p), ("ext", C.c_void_p),
                ("ratio", C.c_void_p), ("open", C.c_void_p), ("cap_rows", C.c_int64)]


class PartialGenotypes(NamedTuple):
    """What Engine.genotype_partial found: one row per (read, locus) of n reads and m loci, all on the engine's device.  include/mtr_hip.h defines
    every column.  A row with open set says "at least ext[2] copies": the repeat runs off the read."""
    partial: "object"     # uint8 [n, m]: 1 = the read does not span the locus and holds one of its flanks; 0 = every other column of the row is 0
    slot: "object"        # uint8 [n, m]: the flank the extension starts from: 0 = A, 1 = B, 2 = rc A, 3 = rc B
    flank_dist: "object"  # int32 [n, m]: that flank's edit distance
    window: "object"      # int32 [n, m, 2]: the extension runs in read[lo:hi], from lo for slots 0 and 3, from hi for slots 1 and 2
    ext: "object"         # int32 [n, m, 6]: ext_len, motif_bases, copies, matches, score, tail
    ratio: "object"       # float32 [n, m]: matches / ext_len
    open: "object"        # uint8 [n, m]: 1 = partial and tail <= max_tail: copies is a lower bound


class CPartialCatalogDst(C.Structure):
    """mtr_partial_catalog_dst: device pointers of the partial catalogue genotype's read and locus columns, and the partial genotype's columns"""
    _fields_ = [("read", C.c_void_p), ("locus", C.c_void_p), ("rows", CPartialDst)]


class CCatalogInfo(C.Structure):
    """mtr_catalog_info"""
    _fields_ = [("n_loci", C.c_int32), ("max_flank_dist", C.c_int32), ("seed_len", C.c_int32), ("filter_bits", C.c_int32), ("entries", C.c_int64),
                ("distinct_codes", C.c_int64), ("table_slots", C.c_int64), ("first_long_motif", C.c_int64), ("device_bytes", C.c_int64)]


class CCatalogDump(C.Structure):
    """mtr_catalog_dump (include/mtr_hip_test.h): host copies of a prepared catalogue's device tables, malloc'ed by the library"""
    _fields_ = [(k, C.c_int64) for k in ("filter_words", "table_slots", "entries", "n_slots", "unit_bytes", "n_loci")] + \
               [(k, C.c_void_p) for k in ("filter", "key", "run", "ent", "plen", "masks", "units", "unit_off", "unit_bits", "variant_bits", "ulen")]


class CatalogInfo(NamedTuple):
    """mtr_catalog_info: what a prepared catalogue holds"""
    n_loci: int
    max_flank_dist: int
    seed_len: int
    filter_bits: int          # the filter has 2^filter_bits bits
    entries: int              # distinct (code, slot) pairs
    distinct_codes: int
    table_slots: int
    first_long_motif: int     # the first locus whose motif exceeds 32 bases (genotype_partial_prepared refuses the catalogue), or -1
    device_bytes: int


class Catalog:
    """mtr_catalog: a locus list prepared once on the GPU (Engine.build_catalog) - the seed index, the flank masks and the motif tables that
    Engine.genotype_catalog and Engine.genotype_partial_catalog rebuild per call.  Immutable; any Engine on the same device may use it, and it
    outlives the Engine that built it.  close() frees its device memory (no call may be using it); it closes when collected, as FileState."""

    def __init__(self, lib, handle, device: int):
        self.lib, self.h, self.device = lib, handle, device
        ci = CCatalogInfo()
        st = lib.mtr_catalog_info_get(handle, C.byref(ci))
        if st != 0:
            raise MtrError(f"mtr_catalog_info_get: {STATUS.get(st, st)}")
        self.info = CatalogInfo(*(int(getattr(ci, f[0])) for f in CCatalogInfo._fields_))

    n_loci = property(lambda self: self.info.n_loci)
    max_flank_dist = property(lambda self: self.info.max_flank_dist)
    seed_len = property(lambda self: self.info.seed_len)

    def _handle(self):
        if not self.h:
            raise MtrError("the catalogue is closed")
        return self.h

    def close(self):
        if self.h:
            self.lib.mtr_catalog_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SparsePartialGenotypes(NamedTuple):
    """What Engine.genotype_partial_catalog found: the R rows of PartialGenotypes with partial = 1, as a list sorted by (read, locus), all on the
    engine's device.  include/mtr_hip.h defines every column.  Several batches' results are joined with torch.cat per column after the batch's
    first read's index has been added to `read` (and n_reads summed): the joined rows stay sorted."""
    n_reads: int
    n_loci: int
    read: "object"        # int32 [R]
    locus: "object"       # int32 [R]
    partial: "object"     # uint8 [R]: 1
    slot: "object"        # uint8 [R]
    flank_dist: "object"  # int32 [R]
    window: "object"      # int32 [R, 2]
    ext: "object"         # int32 [R, 6]
    ratio: "object"       # float32 [R]
    open: "object"        # uint8 [R]
    candidates: int       # the (read, locus) candidates the seeds left to be verified

    def to_dense(self) -> "PartialGenotypes":
        """the same rows as Engine.genotype_partial returns them, zeros where a row is not partial (n_reads x n_loci rows: small shapes)"""
        import torch

        n, m = self.n_reads, self.n_loci
        at = self.read.long() * m + self.locus.long()
        cols = []
        for c in self[4:11]:
            full = torch.zeros((n * m,) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device)
            full[at] = c
            cols.append(full.reshape((n, m) + tuple(c.shape[1:])))
        return PartialGenotypes(*cols)


class PartialSupport(NamedTuple):
    """What partial_support makes of a PartialGenotypes, per locus"""
    n_partial: "object"   # int64 [m]: partial rows
    n_open: "object"      # int64 [m]: open rows
    max_copies: "object"  # int32 [m]: the largest copies among the open rows with ratio >= min_ratio, 0 without one
    n_beyond: "object"    # int64 [m], or None without calls: those rows whose copies exceed the larger called allele


class CAlleleParams(C.Structure):
    """mtr_allele_params: what supports a locus and which splits are admissible"""
    _fields_ = [("measure", C.c_int32), ("min_ratio", C.c_float), ("min_support", C.c_int32), ("min_percent", C.c_int32), ("min_sep", C.c_int32)]


class CAlleleCallsDst(C.Structure):
    """mtr_allele_calls_dst: device pointers of the allele calls' columns and their capacities"""
    _fields_ = [("support_off", C.c_void_p), ("value", C.c_void_p), ("read", C.c_void_p), ("allele", C.c_void_p), ("zygosity", C.c_void_p),
                ("call", C.c_void_p), ("call_support", C.c_void_p), ("cost", C.c_void_p), ("cap_loci", C.c_int64), ("cap_support", C.c_int64)]


class AlleleCalls(NamedTuple):
    """What Engine.call_alleles made of the genotype rows of n reads and m loci: per locus its S_l supporting reads sorted by (value, read) -
    S of them in all - and the one or two alleles they split into, all on the engine's device.  include/mtr_hip.h defines every column."""
    support_off: "object"   # int64 [m + 1]: locus l's supporting reads are entries support_off[l] .. support_off[l + 1]
    value: "object"         # int32 [S]: copies or bases, ascending within a locus
    read: "object"          # int32 [S]: the read of each value, ascending among equal values
    allele: "object"        # uint8 [S]: 0 = the entry belongs to the first (or only) allele, 1 = to the second
    zygosity: "object"      # uint8 [m]: 0 = too little support for a call, 1 = one allele, 2 = two
    call: "object"          # int32 [m, 2]: the alleles' values, the lower medians of their entries
    call_support: "object"  # int32 [m, 2]: the alleles' numbers of reads
    cost: "object"          # int64 [m, 2]: the sum of absolute deviations from the median(s) as one allele, and as called


class CWindowsDst(C.Structure):
    """mtr_windows_dst: device pointers of the windows' two columns and their capacities"""
    _fields_ = [("win_off", C.c_void_p), ("win_bases", C.c_void_p), ("cap_rows", C.c_int64), ("cap_bases", C.c_int64)]


class GenotypeWindows(NamedTuple):
    """What Engine.genotype_windows cut out of the resident batch: row r's oriented window is bases[off[r]:off[r + 1]], codes 0..3, the read's
    window for orientation 0 and its reverse complement for orientation 1 - every window reads in the locus' direction."""
    off: "object"     # int64 [R + 1]
    bases: "object"   # uint8 [T]


class CConsensusSrc(C.Structure):
    """mtr_consensus_src: device pointers of the rows, their windows and the calls, and their sizes"""
    _fields_ = [("row_read", C.c_void_p), ("row_locus", C.c_void_p), ("win_off", C.c_void_p), ("win_bases", C.c_void_p), ("support_off", C.c_void_p), ("read", C.c_void_p),
                ("allele", C.c_void_p), ("zygosity", C.c_void_p), ("n_rows", C.c_int64), ("n_bases", C.c_int64), ("n_support", C.c_int64), ("n_loci", C.c_int32)]


class CConsensusDst(C.Structure):
    """mtr_consensus_dst: device pointers of the consensus' columns and their capacities"""
    _fields_ = [("cons_off", C.c_void_p), ("bases", C.c_void_p), ("votes", C.c_void_p), ("backbone_read", C.c_void_p), ("backbone_len", C.c_void_p), ("members", C.c_void_p),
                ("aligned", C.c_void_p), ("skipped", C.c_void_p), ("cap_alleles", C.c_int64), ("cap_bases", C.c_int64)]


class AlleleConsensus(NamedTuple):
    """What Engine.allele_consensus voted: one group per allele index 2 * locus + a of m loci, all on the engine's device.  include/mtr_hip.h
    defines every column.  Allele A's sequence is bases[off[A]:off[A + 1]]; an allele that was not called has an empty span."""
    off: "object"            # int64 [2m + 1]
    bases: "object"          # uint8 [T]: codes 0..3
    votes: "object"          # int32 [T]: the votes each emitted base had
    backbone_read: "object"  # int32 [2m]: the read whose window the members were aligned to, -1 without an allele
    backbone_len: "object"   # int32 [2m]
    members: "object"        # int32 [2m]: the allele's supporting reads, the backbone among them
    aligned: "object"        # int32 [2m]: the members aligned to the backbone
    skipped: "object"        # int32 [2m]: the members left out (a window or a band beyond the limits)


class CWindowStructureDst(C.Structure):
    """mtr_window_structure_dst: device pointers of the window structure's columns and their capacity"""
    _fields_ = [("seg", C.c_void_p), ("score", C.c_void_p), ("ratio", C.c_void_p), ("skipped", C.c_void_p), ("cap_windows", C.c_int64)]


class WindowStructure(NamedTuple):
    """What Engine.window_structure found: one row per window, all on the engine's device.  include/mtr_hip.h defines every column."""
    seg: "object"      # int32 [N, 4, 4]: per segment start, end, copies, matches; a segment without copies is empty at the next one's start
    score: "object"    # int32 [N]
    ratio: "object"    # float32 [N]: the matches of all segments over the window's length
    skipped: "object"  # uint8 [N]: 1 = the window is longer than WS_MAX_WINDOW and every other column of the row is 0


class CWindowEditsDst(C.Structure):
    """mtr_window_edits_dst: device pointers of the window edits' columns and their capacities"""
    _fields_ = [("off", C.c_void_p), ("edits", C.c_void_p), ("seg", C.c_void_p), ("score", C.c_void_p), ("skipped", C.c_void_p), ("cap_windows", C.c_int64),
                ("cap_edits", C.c_int64)]


class WindowEdits(NamedTuple):
    """What Engine.window_edits found, all on the engine's device.  include/mtr_hip.h ("window edits") defines every column."""
    off: "object"      # int64 [N + 1]: window w's edits are rows off[w] .. off[w + 1] of edits
    edits: "object"    # int32 [T, 6]: pos, segment, copy, column, kind (0 substitution, 1 insertion, 2 deletion), base - in path order
    seg: "object"      # int32 [N, 4, 4]: Engine.window_structure's seg of the same input
    score: "object"    # int32 [N]: its score
    skipped: "object"  # uint8 [N]: its skipped; such a window has no edits


class CSeqParams(C.Structure):
    """mtr_seq_params: where the distances saturate and which medoid pairs are admissible"""
    _fields_ = [("max_dist", C.c_int32), ("min_support", C.c_int32), ("min_percent", C.c_int32), ("min_sep", C.c_int32), ("min_gain", C.c_int32)]


class CSeqCallsDst(C.Structure):
    """mtr_seq_calls_dst: device pointers of the sequence calls' columns - mtr_allele_calls_dst's eight first - and their capacities"""
    _fields_ = [("support_off", C.c_void_p), ("value", C.c_void_p), ("read", C.c_void_p), ("allele", C.c_void_p), ("zygosity", C.c_void_p),
                ("call", C.c_void_p), ("call_support", C.c_void_p), ("cost", C.c_void_p), ("medoid", C.c_void_p), ("dist_to_medoid", C.c_void_p),
                ("skipped", C.c_void_p), ("pair_off", C.c_void_p), ("dist", C.c_void_p), ("cap_loci", C.c_int64), ("cap_support", C.c_int64), ("cap_pairs", C.c_int64)]


class SequenceCalls(NamedTuple):
    """What Engine.call_alleles_by_sequence made of a locus' supporting reads' windows, all on the engine's device.  include/mtr_hip.h
    ("sequence allele calls") defines every column."""
    calls: AlleleCalls          # the split in call_alleles' shape: allele_consensus, format_allele_calls and partial_support take it unchanged
    medoid: "object"            # int32 [m, 2]: the medoids' reads, -1 without one
    dist_to_medoid: "object"    # int32 [S]: each entry's distance to its own allele's medoid
    skipped: "object"           # uint8 [m]: 1 = more than SEQ_MAX_MEMBERS supporting reads, no pairs computed, zygosity 0
    pair_off: "object"          # int64 [m + 1]: locus l owns S_l (S_l - 1) / 2 pairs, none when skipped
    dist: "object"              # uint8 [P]: the upper triangle of D, row-major, pair (t < u) at pair_off[l] + t * S_l - t (t + 1) / 2 + (u - t - 1)


class CGqParams(C.Structure):
    """mtr_gq_params: the band and where a base's weight, a gap's cost and a read's score saturate"""
    _fields_ = [("band_extra", C.c_int32), ("qual_cap", C.c_int32), ("gap_cap", C.c_int32), ("read_cap", C.c_int32)]


class CGqDst(C.Structure):
    """mtr_gq_dst: device pointers of the genotype quality's nine columns and their capacities"""
    _fields_ = [("score", C.c_void_p), ("best", C.c_void_p), ("margin", C.c_void_p), ("raw", C.c_void_p), ("pl", C.c_void_p), ("gt", C.c_void_p), ("gq", C.c_void_p),
                ("scored", C.c_void_p), ("unscored", C.c_void_p), ("cap_support", C.c_int64), ("cap_loci", C.c_int64)]


class GenotypeQuality(NamedTuple):
    """What Engine.genotype_quality made of every supporting read's score against both allele sequences, all on the engine's device.
    include/mtr_hip.h ("genotype quality") defines every column."""
    score: "object"     # int32 [S, 2]: the entry's quality-weighted distance to allele 0's and allele 1's sequence, -1 where there is none
    best: "object"      # uint8 [S]: the allele the entry fits better, its own on a tie or without scores
    margin: "object"    # int32 [S]: |score 0 - score 1|, 0 without two scores
    raw: "object"       # int64 [m, 3]: the Phred-scaled sums for the genotypes 0/0, 0/1, 1/1; -1 where there is no such genotype
    pl: "object"        # int64 [m, 3]: raw less its minimum (a VCF's PL)
    gt: "object"        # uint8 [m]: 0 = 0/0, 1 = 0/1, 2 = 1/1, 255 = no call
    gq: "object"        # int64 [m]: the least pl of the two other genotypes (a VCF's GQ), -1 without two alleles
    scored: "object"    # int32 [m]: the locus' entries that were scored
    unscored: "object"  # int32 [m]: those that were not (a window, an allele or a band beyond the limits)


class CFastaInfo(C.Structure):
    """mtr_fasta_info: what a FASTA file in device memory holds"""
    _fields_ = [("n_reads", C.c_int32), ("end", C.c_int32), ("bad_char", C.c_int32), ("reserved", C.c_int32),
                ("end_pos", C.c_int64), ("n_bases", C.c_int64), ("id_bytes", C.c_int64)]


class CFastaDst(C.Structure):
    """mtr_fasta_dst: device pointers of the parsed reads' columns and their capacities"""
    _fields_ = [("text", C.c_void_p), ("offsets", C.c_void_p), ("lens", C.c_void_p), ("ids", C.c_void_p), ("id_off", C.c_void_p),
                ("cap_text", C.c_int64), ("cap_reads", C.c_int64), ("cap_id_bytes", C.c_int64)]


class Fasta(NamedTuple):
    """The reads of a FASTA file parsed on the device (Engine.parse_fasta_device / upload_fasta_device): those before the stop."""
    text: "object"        # uint8 [n_bases] on the engine's device: the reads' bases, the file's own bytes (None after upload_fasta_device)
    offsets: "object"     # int64 numpy [n_reads]: read i is text[offsets[i]:offsets[i] + lens[i]]
    lens: "object"        # int32 numpy [n_reads]
    ids: list             # bytes per read: what its header holds behind '>'
    end: str              # why the input ended: "eof", "empty" (a record without bases), "bad" (character), "toolong" (a record of 1 000 000 bases);
                          # FASTQ: "format" too; a window with more behind it (more=True) that holds no stop: "more"
    bad_char: "object"    # the character of end == "bad" as bytes, else None
    end_pos: int          # the stop's position in the file (its length when the file ended); "more": where the next window starts


class CKernelTime(C.Structure):
    _fields_ = [("ms", C.c_float), ("launches", C.c_int32)]


class Record(NamedTuple):
    """The 15 per-repeat arguments of insert_an_alignment_into_set (reference mTR.h:151-168)."""
    rep_start: int
    rep_end: int
    repeat_len: int
    rep_period: int
    num_freq_unit: int
    num_matches: int
    num_mismatches: int
    num_insertions: int
    num_deletions: int
    kmer: int
    match_gain: int
    mismatch_penalty: int
    indel_penalty: int
    unit: str
    unit_score: tuple


_lib = None


def load_library(path: str = LIB_PATH):
    """dlopen libmtr_hip.so; raises if it has not been built (python -m mtr_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise MtrError(f"{path} is missing: build it with `python -m mtr_amd.build` (hipcc, gfx950); there is no CPU fallback")
    lib = C.CDLL(path)
    P = C.POINTER
    lib.mtr_create.argtypes = [C.c_int, C.c_int, C.c_float, P(C.c_void_p)]
    lib.mtr_create.restype = C.c_int
    lib.mtr_destroy.argtypes = [C.c_void_p]
    lib.mtr_destroy.restype = None
    lib.mtr_last_error.argtypes = [C.c_void_p]
    lib.mtr_last_error.restype = C.c_char_p
    lib.mtr_abi_version.restype = C.c_int
    lib.mtr_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, P(P(CRecord)), P(P(C.c_int32)), P(C.c_int64)]
    lib.mtr_process_batch.restype = C.c_int
    lib.mtr_free_results.argtypes = [C.c_void_p, C.c_void_p]
    lib.mtr_free_results.restype = None
    lib.mtr_upload_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mtr_upload_batch.restype = C.c_int
    lib.mtr_run_resident.argtypes = [C.c_void_p]
    lib.mtr_run_resident.restype = C.c_int
    lib.mtr_file_state_create.argtypes = [P(C.c_void_p)]
    lib.mtr_file_state_create.restype = C.c_int
    lib.mtr_file_state_destroy.argtypes = [C.c_void_p]
    lib.mtr_file_state_destroy.restype = None
    lib.mtr_upload_batch_in_file.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mtr_upload_batch_in_file.restype = C.c_int
    lib.mtr_file_state_skip.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mtr_file_state_skip.restype = C.c_int
    lib.mtr_run_resident_async.argtypes = [C.c_void_p]
    lib.mtr_run_resident_async.restype = C.c_int
    lib.mtr_wait.argtypes = [C.c_void_p]
    lib.mtr_wait.restype = C.c_int
    lib.mtr_test_last_mode.argtypes = [C.c_void_p]
    lib.mtr_test_last_mode.restype = C.c_int32
    lib.mtr_fetch_results.argtypes = [C.c_void_p, P(P(CRecord)), P(P(C.c_int32)), P(C.c_int64)]
    lib.mtr_fetch_results.restype = C.c_int
    lib.mtr_get_kernel_times.argtypes = [C.c_void_p, P(CKernelTime), C.c_int32]
    lib.mtr_get_kernel_times.restype = C.c_int
    lib.mtr_alignments.argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), C.c_void_p, P(P(C.c_uint8)), P(P(C.c_int64)), P(P(C.c_int32))]
    lib.mtr_alignments.restype = C.c_int
    lib.mtr_get_counters.argtypes = [C.c_void_p, P(C.c_int64), C.c_int32]
    lib.mtr_get_counters.restype = C.c_int
    lib.mtr_test_ranges.argtypes = [C.c_void_p, P(P(C.c_int32)), P(P(C.c_int32)), P(P(C.c_int32)), P(P(C.c_int32)), P(P(C.c_uint64)), P(C.c_int64)]
    lib.mtr_test_ranges.restype = C.c_int
    lib.mtr_test_ranges_parts.argtypes = lib.mtr_test_ranges.argtypes
    lib.mtr_test_ranges_parts.restype = C.c_int
    lib.mtr_test_wrap_dp.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 9
    lib.mtr_test_wrap_dp.restype = C.c_int
    lib.mtr_test_wrap_dp_pass.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 10
    lib.mtr_test_wrap_dp_pass.restype = C.c_int
    lib.mtr_test_polish.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 9
    lib.mtr_test_polish.restype = C.c_int
    lib.mtr_test_revise.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 3
    lib.mtr_test_revise.restype = C.c_int
    lib.mtr_upload_batch_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mtr_upload_batch_packed.restype = C.c_int
    lib.mtr_upload_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.mtr_upload_batch_device.restype = C.c_int
    lib.mtr_fetch_results_packed.argtypes = [C.c_void_p, C.c_int32, P(C.c_void_p), P(C.c_int64), P(C.c_void_p), P(C.c_int64)]
    lib.mtr_fetch_results_packed.restype = C.c_int
    lib.mtr_export_packed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, P(C.c_int64), P(C.c_int64)]
    lib.mtr_export_packed_device.restype = C.c_int
    lib.mtr_report_device.argtypes = [C.c_void_p, P(CReportDst), C.c_void_p, P(C.c_int64), P(C.c_int64)]
    lib.mtr_report_device.restype = C.c_int
    lib.mtr_report_alignments_device.argtypes = [C.c_void_p, P(CReportAlignDst), P(C.c_int64), P(C.c_int64)]
    lib.mtr_report_alignments_device.restype = C.c_int
    lib.mtr_report_text_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, P(CReportTextDst), P(C.c_int64)]
    lib.mtr_report_text_device.restype = C.c_int
    lib.mtr_report_motifs_device.argtypes = [C.c_void_p, P(CReportMotifDst), P(C.c_int64), P(C.c_int64), P(C.c_int64)]
    lib.mtr_report_motifs_device.restype = C.c_int
    lib.mtr_test_unit_motifs.argtypes = ([C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int64, P(P(C.c_uint8))] + [P(P(C.c_int32))] * 3 +
                                         [P(C.c_int64), P(P(C.c_int64)), P(P(C.c_uint8))] + [P(P(C.c_int32))] * 3 + [P(P(C.c_int64))] * 2)
    lib.mtr_test_unit_motifs.restype = C.c_int
    lib.mtr_search_motifs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [P(CMotifHitsDst), P(C.c_int64)]
    lib.mtr_search_motifs_device.restype = C.c_int
    lib.mtr_search_motif_loci_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [P(C.c_int64), P(C.c_int64)]
    lib.mtr_search_motif_loci_device.restype = C.c_int
    lib.mtr_motif_loci_copy_device.argtypes = [C.c_void_p, P(CMotifLociDst)]
    lib.mtr_motif_loci_copy_device.restype = C.c_int
    lib.mtr_search_flanks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, P(CFlankHitsDst), P(C.c_int64)]
    lib.mtr_search_flanks_device.restype = C.c_int
    lib.mtr_genotype_loci_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [P(CGenotypesDst), P(C.c_int64)]
    lib.mtr_genotype_loci_device.restype = C.c_int
    lib.mtr_genotype_catalog_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [P(C.c_int64), P(C.c_int64)]
    lib.mtr_genotype_catalog_device.restype = C.c_int
    lib.mtr_genotype_catalog_copy_device.argtypes = [C.c_void_p, P(CCatalogDst)]
    lib.mtr_genotype_catalog_copy_device.restype = C.c_int
    lib.mtr_genotype_partial_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [P(CPartialDst), P(C.c_int64)]
    lib.mtr_genotype_partial_device.restype = C.c_int
    lib.mtr_genotype_partial_catalog_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [P(C.c_int64), P(C.c_int64)]
    lib.mtr_genotype_partial_catalog_device.restype = C.c_int
    lib.mtr_genotype_partial_catalog_copy_device.argtypes = [C.c_void_p, P(CPartialCatalogDst)]
    lib.mtr_genotype_partial_catalog_copy_device.restype = C.c_int
    if hasattr(lib, "mtr_catalog_create"):      # (a build from before the prepared catalogue, A/B'd through MTR_LIB, has none of these: using one raises there)
        lib.mtr_catalog_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p)]
        lib.mtr_catalog_create.restype = C.c_int
        lib.mtr_catalog_destroy.argtypes = [C.c_void_p]
        lib.mtr_catalog_destroy.restype = None
        lib.mtr_catalog_info_get.argtypes = [C.c_void_p, P(CCatalogInfo)]
        lib.mtr_catalog_info_get.restype = C.c_int
        lib.mtr_genotype_catalog_prepared_device.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 3 + [P(C.c_int64), P(C.c_int64)]
        lib.mtr_genotype_catalog_prepared_device.restype = C.c_int
        lib.mtr_genotype_partial_catalog_prepared_device.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [P(C.c_int64), P(C.c_int64)]
        lib.mtr_genotype_partial_catalog_prepared_device.restype = C.c_int
        lib.mtr_test_catalog_dump.argtypes = [C.c_void_p, C.c_void_p, P(CCatalogDump)]
        lib.mtr_test_catalog_dump.restype = C.c_int
        lib.mtr_test_catalog_build_stats.argtypes = [C.c_void_p, P(C.c_double)]
        lib.mtr_test_catalog_build_stats.restype = C.c_int
    lib.mtr_call_alleles_device.argtypes = [C.c_void_p, P(CGenotypesDst), C.c_int64, C.c_int32, P(CAlleleParams), C.c_void_p, P(CAlleleCallsDst), P(C.c_int64)]
    lib.mtr_call_alleles_device.restype = C.c_int
    lib.mtr_call_alleles_rows_device.argtypes = [C.c_void_p, P(CGenotypesDst), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(CAlleleParams), C.c_void_p, P(CAlleleCallsDst),
                                                 P(C.c_int64)]
    lib.mtr_call_alleles_rows_device.restype = C.c_int
    if hasattr(lib, "mtr_allele_consensus_device"):      # (a build from before the consensus, A/B'd through MTR_LIB, has neither: using one raises there)
        lib.mtr_extract_windows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, P(CWindowsDst), P(C.c_int64)]
        lib.mtr_extract_windows_device.restype = C.c_int
        lib.mtr_allele_consensus_device.argtypes = [C.c_void_p, P(CConsensusSrc), C.c_int32, C.c_void_p, P(CConsensusDst), P(C.c_int64)]
        lib.mtr_allele_consensus_device.restype = C.c_int
    if hasattr(lib, "mtr_window_structure_device"):      # (likewise a build from before the window structure)
        lib.mtr_window_structure_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                    C.c_int32, C.c_int32, C.c_int32, C.c_void_p, P(CWindowStructureDst)]
        lib.mtr_window_structure_device.restype = C.c_int
    if hasattr(lib, "mtr_window_edits_device"):          # (likewise a build from before the window edits)
        lib.mtr_window_edits_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_void_p, P(C.c_int64)]
        lib.mtr_window_edits_device.restype = C.c_int
        lib.mtr_window_edits_copy_device.argtypes = [C.c_void_p, P(CWindowEditsDst)]
        lib.mtr_window_edits_copy_device.restype = C.c_int
        lib.mtr_test_window_edits_rounds.argtypes = [C.c_void_p, P(C.c_int32)]
        lib.mtr_test_window_edits_rounds.restype = C.c_int
    if hasattr(lib, "mtr_call_alleles_sequence_device"):          # (likewise a build from before the sequence calls)
        lib.mtr_call_alleles_sequence_device.argtypes = [C.c_void_p, P(CConsensusSrc), C.c_void_p, P(CSeqParams), C.c_void_p, P(C.c_int64), P(C.c_int64)]
        lib.mtr_call_alleles_sequence_device.restype = C.c_int
        lib.mtr_call_alleles_sequence_copy_device.argtypes = [C.c_void_p, P(CSeqCallsDst)]
        lib.mtr_call_alleles_sequence_copy_device.restype = C.c_int
    if hasattr(lib, "mtr_allele_consensus_quality_device"):       # (likewise a build from before the qualities)
        lib.mtr_keep_qualities.argtypes = [C.c_void_p, C.c_int32]
        lib.mtr_attach_qualities_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.mtr_qualities_resident.argtypes = [C.c_void_p, P(C.c_int64)]
        lib.mtr_extract_window_qualities_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
        lib.mtr_allele_consensus_quality_device.argtypes = [C.c_void_p, P(CConsensusSrc), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, P(CConsensusDst), P(C.c_int64)]
        for name in ("mtr_keep_qualities", "mtr_attach_qualities_device", "mtr_qualities_resident", "mtr_extract_window_qualities_device", "mtr_allele_consensus_quality_device"):
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "mtr_genotype_quality_device"):               # (likewise a build from before the genotype quality)
        lib.mtr_genotype_quality_device.argtypes = [C.c_void_p, P(CConsensusSrc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, P(CGqParams), C.c_void_p, P(CGqDst)]
        lib.mtr_genotype_quality_device.restype = C.c_int
    lib.mtr_test_catalog_stats.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_double)]
    lib.mtr_test_catalog_stats.restype = C.c_int
    lib.mtr_test_partial_catalog_stats.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_double)]
    lib.mtr_test_partial_catalog_stats.restype = C.c_int
    lib.mtr_parse_fasta_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, P(CFastaDst), P(CFastaInfo)]
    lib.mtr_parse_fasta_device.restype = C.c_int
    lib.mtr_upload_fasta_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, P(CFastaInfo)]
    lib.mtr_upload_fasta_device.restype = C.c_int
    lib.mtr_upload_batch_device_in_file.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.mtr_upload_batch_device_in_file.restype = C.c_int
    lib.mtr_upload_fasta_device_in_file.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, P(CFastaInfo)]
    lib.mtr_upload_fasta_device_in_file.restype = C.c_int
    lib.mtr_file_state_skip_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.mtr_file_state_skip_device.restype = C.c_int
    lib.mtr_test_file_tail.argtypes = [C.c_void_p, P(P(C.c_uint16)), P(P(C.c_int64)), P(P(C.c_uint8))]
    lib.mtr_test_file_tail.restype = C.c_int
    for name in ("mtr_parse_fastq_device", "mtr_upload_fastq_device", "mtr_upload_fastq_device_in_file"):       # as their FASTA twins
        twin = getattr(lib, name.replace("fastq", "fasta"))
        getattr(lib, name).argtypes, getattr(lib, name).restype = twin.argtypes, twin.restype
    for fmt in ("fasta", "fastq"):                              # more_follows behind n_bytes; the upload takes the file state, NULL or not
        parse, upload = getattr(lib, f"mtr_parse_{fmt}_device_window"), getattr(lib, f"mtr_upload_{fmt}_device_window")
        parse.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, P(CFastaDst), P(CFastaInfo)]
        upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, P(CFastaInfo)]
        parse.restype = upload.restype = C.c_int
    lib.mtr_fasta_index.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mtr_fasta_index.restype = C.c_int
    lib.mtr_test_report_lines.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [P(P(C.c_uint8)), P(P(C.c_int64))]
    lib.mtr_test_report_lines.restype = C.c_int
    lib.mtr_test_chain.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(P(C.c_int32)), P(P(C.c_int32))]
    lib.mtr_test_chain.restype = C.c_int
    lib.mtr_unpack_records.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.mtr_unpack_records.restype = C.c_int
    lib.mtr_pack_records.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    lib.mtr_pack_records.restype = C.c_int64
    lib.mtr_get_first_failed_read.argtypes = [C.c_void_p, P(C.c_int32)]
    lib.mtr_get_first_failed_read.restype = C.c_int
    lib.mtr_set_trace.argtypes = [C.c_void_p, C.c_int32]
    lib.mtr_set_trace.restype = C.c_int
    lib.mtr_get_trace.argtypes = [C.c_void_p, P(P(C.c_int32)), P(C.c_int64)]
    lib.mtr_get_trace.restype = C.c_int
    _lib = lib
    return lib


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _flatten(reads: Sequence[np.ndarray]):
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.zeros(len(reads), dtype=np.int64)
    if len(reads) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    bases = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]) if len(reads) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(bases), offs, lens


def _host_ints(a, dtype, what: str) -> np.ndarray:
    if hasattr(a, "detach"):                   # a torch tensor: it must be on the CPU
        if a.device.type != "cpu":
            raise MtrError(f"{what} must be a host array, got a tensor on {a.device}")
        a = a.detach().numpy()
    a = np.asarray(a)
    if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
        raise MtrError(f"{what} must be a 1-D integer array, got shape {a.shape} dtype {a.dtype}")
    out = np.ascontiguousarray(a, dtype=dtype)
    if not np.array_equal(out, a):
        raise MtrError(f"{what} does not fit {np.dtype(dtype).name}")
    return out


def device_input_args(text, offsets, lens, device: int):
    """The checks of Engine.upload_device, made before the library is called: text a contiguous 1-D torch.uint8 tensor on
    cuda:device, offsets / lens host integer arrays of one length, every read 1..MAX_READ_LENGTH bytes inside text.
    Returns (offsets int64, lens int32) as contiguous numpy arrays; raises MtrError."""
    import torch

    if not isinstance(text, torch.Tensor):
        raise MtrError(f"text must be a torch.Tensor, got {type(text).__name__}")
    if text.dtype != torch.uint8:
        raise MtrError(f"text must have dtype torch.uint8, got {text.dtype}")
    if text.dim() != 1 or not text.is_contiguous():
        raise MtrError(f"text must be a contiguous 1-D tensor, got shape {tuple(text.shape)} strides {text.stride()}")
    offs = _host_ints(offsets, np.int64, "offsets")
    ln = _host_ints(lens, np.int32, "lens")
    if len(offs) != len(ln) or len(ln) == 0:
        raise MtrError(f"offsets ({len(offs)}) and lens ({len(ln)}) must have the same, non-zero length")
    if (ln <= 0).any() or (ln > MAX_READ_LENGTH).any():
        i = int(np.argmax((ln <= 0) | (ln > MAX_READ_LENGTH)))
        raise MtrError(f"read {i}: length {int(ln[i])} outside 1..{MAX_READ_LENGTH}")
    past = (offs < 0) | (offs > text.numel() - ln.astype(np.int64))
    if past.any():
        i = int(np.argmax(past))
        raise MtrError(f"read {i}: bytes {int(offs[i])} .. +{int(ln[i])} outside the text of {text.numel()} bytes")
    if text.device.type != "cuda":
        raise MtrError(f"text must be a GPU tensor, got a tensor on {text.device}")
    if text.device.index != device:
        raise MtrError(f"text is on {text.device}, the engine on cuda:{device}")
    return offs, ln


def fasta_input_args(buf, device: int) -> None:
    """The checks of Engine.parse_fasta_device / upload_fasta_device and their FASTQ twins, made before the library is called: buf
    a contiguous 1-D torch.uint8 tensor on cuda:device (the bytes of a FASTA or FASTQ file; it may be empty).  Raises MtrError."""
    import torch

    if not isinstance(buf, torch.Tensor):
        raise MtrError(f"buf must be a torch.Tensor, got {type(buf).__name__}")
    if buf.dtype != torch.uint8:
        raise MtrError(f"buf must have dtype torch.uint8, got {buf.dtype}")
    if buf.dim() != 1 or not buf.is_contiguous():
        raise MtrError(f"buf must be a contiguous 1-D tensor, got shape {tuple(buf.shape)} strides {buf.stride()}")
    if buf.device.type != "cuda":
        raise MtrError(f"buf must be a GPU tensor, got a tensor on {buf.device}")
    if buf.device.index != device:
        raise MtrError(f"buf is on {buf.device}, the engine on cuda:{device}")


def genotype_rows_args(gt, device: int):
    """The checks of Engine.call_alleles on its genotype rows, made before the library is called: gt.spanning a contiguous 2-D torch.uint8 tensor
    [n, m] with n, m >= 1, gt.window [n, m, 2] int32, gt.fields [n, m, 8] int32, gt.ratio [n, m] float32, all contiguous and on cuda:device (a
    Genotypes, or anything with these four attributes: the other columns are not read).  Returns (n, m); raises MtrError."""
    import torch

    sp = getattr(gt, "spanning", None)
    if not isinstance(sp, torch.Tensor):
        raise MtrError(f"gt.spanning must be a torch.Tensor, got {type(sp).__name__}")
    if sp.dtype != torch.uint8:
        raise MtrError(f"gt.spanning must have dtype torch.uint8, got {sp.dtype}")
    if sp.dim() != 2 or sp.shape[0] < 1 or sp.shape[1] < 1:
        raise MtrError(f"gt.spanning must be [n, m] with n, m >= 1, got shape {tuple(sp.shape)}")
    n, m = int(sp.shape[0]), int(sp.shape[1])
    cols = (("spanning", sp, torch.uint8, (n, m)), ("window", getattr(gt, "window", None), torch.int32, (n, m, 2)),
            ("fields", getattr(gt, "fields", None), torch.int32, (n, m, 8)), ("ratio", getattr(gt, "ratio", None), torch.float32, (n, m)))
    for name, t, dtype, shape in cols:
        if not isinstance(t, torch.Tensor):
            raise MtrError(f"gt.{name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != dtype:
            raise MtrError(f"gt.{name} must have dtype {dtype}, got {t.dtype}")
        if tuple(t.shape) != shape:
            raise MtrError(f"gt.{name} must have shape {shape}, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise MtrError(f"gt.{name} must be contiguous, got strides {t.stride()}")
    if n * m > 2 ** 31 - 1:
        raise MtrError(f"{n} reads x {m} loci are more than 2^31 - 1 rows")
    for name, t, _, _ in cols:
        if t.device != sp.device:
            raise MtrError(f"gt.{name} is on {t.device}, gt.spanning on {sp.device}: the columns must be on one device")
    if sp.device.type != "cuda":
        raise MtrError(f"the genotype rows must be GPU tensors, got tensors on {sp.device}")
    if sp.device.index != device:
        raise MtrError(f"the genotype rows are on {sp.device}, the engine on cuda:{device}")
    return n, m


def sparse_rows_args(sg, device: int):
    """The checks of Engine.call_alleles on a SparseGenotypes, made before the library is called: read, locus (int32 [R]), spanning (uint8 [R]),
    window (int32 [R, 2]), fields (int32 [R, 8]) and ratio (float32 [R]) contiguous torch tensors on the engine's GPU, n_loci >= 1.  Returns
    (R, n_loci); raises MtrError."""
    import torch

    if isinstance(sg.n_loci, bool) or not isinstance(sg.n_loci, (int, np.integer)) or sg.n_loci < 1:
        raise MtrError(f"n_loci must be an integer >= 1, got {sg.n_loci!r}")
    if not isinstance(sg.read, torch.Tensor) or sg.read.dim() != 1:
        raise MtrError("the rows' read column must be a 1-D torch tensor")
    R = int(sg.read.numel())
    want = (("read", torch.int32, (R,)), ("locus", torch.int32, (R,)), ("spanning", torch.uint8, (R,)), ("window", torch.int32, (R, 2)), ("fields", torch.int32, (R, 8)),
            ("ratio", torch.float32, (R,)))
    for name, dtype, shape in want:
        t = getattr(sg, name)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise MtrError(f"the rows' {name} must be a contiguous {dtype} tensor of shape {shape}")
    for name, _, _ in want:
        t = getattr(sg, name)
        if not t.is_cuda:
            raise MtrError(f"the genotype rows must be GPU tensors, got tensors on {t.device}")
        if t.device.index != device:
            raise MtrError(f"the genotype rows are on {t.device}, the engine on cuda:{device}")
    return R, int(sg.n_loci)


def _fasta(info: CFastaInfo, text, offsets, lens, id_off, ids: bytes) -> Fasta:
    return Fasta(text, offsets, lens, [ids[int(id_off[i]):int(id_off[i + 1])] for i in range(info.n_reads)], FASTQ_END[info.end],
                 bytes([info.bad_char & 0xFF]) if info.end == 2 else None, int(info.end_pos))


def pack_ids(ids, n_reads: "int | None" = None):
    """The IDs of a batch as mtr_report_text_device takes them: (bytes uint8 [>= 1], id_off int64 [n + 1]) as contiguous numpy arrays,
    ID i = bytes[id_off[i]:id_off[i + 1]].  ids: one str (encoded as UTF-8) or bytes per read - what the FASTA header holds after '>'.
    n_reads: the number of reads they must name.  Raises MtrError."""
    if isinstance(ids, (str, bytes, bytearray)) or not hasattr(ids, "__len__"):
        raise MtrError(f"ids must be a sequence of str or bytes, one per read, got {type(ids).__name__}")
    if n_reads is not None and len(ids) != n_reads:
        raise MtrError(f"{len(ids)} ids for {n_reads} uploaded reads")
    raw = []
    for i, v in enumerate(ids):
        if isinstance(v, str):
            raw.append(v.encode())
        elif isinstance(v, (bytes, bytearray)):
            raw.append(bytes(v))
        else:
            raise MtrError(f"id {i} must be str or bytes, got {type(v).__name__}")
    off = np.zeros(len(raw) + 1, np.int64)
    if raw:
        off[1:] = np.cumsum([len(b) for b in raw], dtype=np.int64)
    data = np.frombuffer(b"".join(raw) + b"\0", np.uint8)                # (never empty: the library takes no NULL ids)
    return np.ascontiguousarray(data), off


class Engine:
    """One context per GPU (mtr_create).  manhattan=False is the reference's -p; min_match_ratio its -m.

    The device-input methods (upload_device, process_device, export_tensor) use torch: import torch BEFORE the first Engine
    is created.  torch ships its own HIP runtime under the same soname as the one libmtr_hip.so links, and whichever loads
    first serves both; loaded second, torch finds no GPU."""

    def __init__(self, device: int = 0, manhattan: bool = True, min_match_ratio: float = 0.6):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.mtr_create(device, 1 if manhattan else 0, C.c_float(min_match_ratio), C.byref(h))
        if st != 0:
            raise MtrError(f"mtr_create failed: {STATUS.get(st, st)} (a HIP device is required; there is no CPU fallback)")
        self.h = h
        self.device = device
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.mtr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, what: str):
        if st != 0:
            raise MtrError(f"{what}: {STATUS.get(st, st)}: {self.lib.mtr_last_error(self.h).decode(errors='replace')}")

    # ---- the batch edge -------------------------------------------------------------------------------
    def upload(self, reads: Sequence[np.ndarray], file_state: "FileState | None" = None):
        """file_state: the reads are the next reads of that file (file-order mode, mtr_upload_batch_in_file)"""
        bases, offs, lens = _flatten(reads)
        self._keep = (bases, offs, lens)
        if file_state is None:
            self._check(self.lib.mtr_upload_batch(self.h, bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(reads)), "mtr_upload_batch")
        else:
            self._check(self.lib.mtr_upload_batch_in_file(self.h, file_state.h, bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(reads)),
                        "mtr_upload_batch_in_file")
        self.n_reads = len(reads)

    def upload_flat(self, bases: np.ndarray, offs: np.ndarray, lens: np.ndarray):
        """mtr_upload_batch on host buffers the caller already holds in the boundary's form (concatenated base codes, offsets, lengths):
        the library packs them to 2 bit/base on the calling thread and copies the image to the device"""
        self._keep = (bases, offs, lens)
        self._check(self.lib.mtr_upload_batch(self.h, bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(lens)), "mtr_upload_batch")
        self.n_reads = len(lens)

    def upload_device(self, text, offsets, lens, codes: bool = False, file_state: "FileState | None" = None):
        """mtr_upload_batch_device: reads as text already on the GPU, packed there by a kernel.
        text: contiguous 1-D torch.uint8 tensor on this engine's device, one byte per base - 'ACGT'/'acgt' (codes=False) or
        0..3 (codes=True); offsets / lens: host int64 / int32 arrays (numpy or CPU tensors).  The library waits for torch's
        current stream (where text was written) by an event; text may be reused once this returns.
        file_state: the reads are the next reads of that file (file-order mode, mtr_upload_batch_device_in_file): the state is
        fed from device memory and keeps its bases there."""
        import torch

        offs, ln = device_input_args(text, offsets, lens, self.device)
        stream = torch.cuda.current_stream(text.device).cuda_stream
        self.n_reads = 0
        if file_state is None:
            self._check(self.lib.mtr_upload_batch_device(self.h, C.c_void_p(text.data_ptr()), text.numel(), offs.ctypes.data, ln.ctypes.data, len(ln),
                                                         TEXT_CODES if codes else TEXT_ASCII, C.c_void_p(stream)), "mtr_upload_batch_device")
        else:
            self._check(self.lib.mtr_upload_batch_device_in_file(self.h, file_state.h, C.c_void_p(text.data_ptr()), text.numel(), offs.ctypes.data,
                                                                 ln.ctypes.data, len(ln), TEXT_CODES if codes else TEXT_ASCII, C.c_void_p(stream)),
                        "mtr_upload_batch_device_in_file")
        self.n_reads = len(ln)

    def parse_fasta_device(self, buf, more: bool = False) -> Fasta:
        """mtr_parse_fasta_device: the bytes of a FASTA file on the GPU parsed there, by the reference reader's rules.
        buf: contiguous 1-D torch.uint8 tensor on this engine's device.  Returns a Fasta whose text is a fresh tensor on that
        device (what upload_device takes) and whose index is on the host; the resident batch is not touched.  The library
        waits for torch's current stream (where buf was written) by an event.
        more=True (mtr_parse_fasta_device_window): buf is the beginning of a longer input.  Without a stop in it the reads are the
        records that a later header closes, end is "more" and end_pos is where the next window starts - the open record's '>'."""
        return self._parse_file_device("mtr_parse_fasta_device", buf, more)

    def parse_fastq_device(self, buf, more: bool = False) -> Fasta:
        """mtr_parse_fastq_device: parse_fasta_device for the bytes of a FASTQ file - strict four-line records, the rules in
        include/mtr_hip.h.  The qualities are checked for their length and dropped; end may be "format" too.
        more=True (mtr_parse_fastq_device_window): the reads are the records whose quality line's LF is in buf; end_pos is the byte
        behind the last of them."""
        return self._parse_file_device("mtr_parse_fastq_device", buf, more)

    def _parse_file_device(self, entry: str, buf, more: bool = False) -> Fasta:
        import torch

        fasta_input_args(buf, self.device)
        dev = torch.device("cuda", self.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        src = C.c_void_p(buf.data_ptr()) if buf.numel() else None
        info = CFastaInfo()
        if more:
            entry += "_window"
            window = getattr(self.lib, entry)
            call = lambda h, src, n, stream, dst, info: window(h, src, n, 1, stream, dst, info)     # noqa: E731
        else:
            call = getattr(self.lib, entry)
        self._check(call(self.h, src, buf.numel(), stream, None, C.byref(info)), entry)
        n, nb, ni = info.n_reads, int(info.n_bases), int(info.id_bytes)
        text = torch.empty(nb, dtype=torch.uint8, device=dev)
        offsets = torch.empty(n, dtype=torch.int64, device=dev)
        lens = torch.empty(n, dtype=torch.int32, device=dev)
        ids = torch.empty(ni, dtype=torch.uint8, device=dev)
        id_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()            # the library writes the tensors on its own stream: torch's earlier use of the memory is done
        ptr = lambda t: t.data_ptr() if t.numel() else None     # noqa: E731
        dst = CFastaDst(ptr(text), ptr(offsets), ptr(lens), ptr(ids), id_off.data_ptr(), nb, n, ni)
        self._check(call(self.h, src, buf.numel(), stream, C.byref(dst), C.byref(info)), entry)
        return _fasta(info, text, offsets.cpu().numpy(), lens.cpu().numpy(), id_off.cpu().numpy(), ids.cpu().numpy().tobytes())

    def upload_fasta_device(self, buf, file_state: "FileState | None" = None, more: bool = False) -> Fasta:
        """mtr_upload_fasta_device + mtr_fasta_index: the reads of a FASTA file on the GPU become the resident batch without a
        host parser; run / fetch / report_* follow as after any upload, and the returned Fasta (text None) carries the ids
        report_text takes.  A stop (end != "eof") does not refuse the upload: the reads before it are uploaded.  No reads: no
        batch is uploaded.  file_state: the reads are the next reads of that file (file-order mode,
        mtr_upload_fasta_device_in_file); the state advances over the uploaded reads.
        more=True (mtr_upload_fasta_device_window): buf is the beginning of a longer input, as in parse_fasta_device; the reads in
        front of end_pos are uploaded.  walk_fasta_device is the loop over a whole file."""
        return self._upload_file_device("mtr_upload_fasta_device", buf, file_state, more)

    def upload_fastq_device(self, buf, file_state: "FileState | None" = None, more: bool = False, keep_quality: bool = False) -> Fasta:
        """mtr_upload_fastq_device(_in_file) + mtr_fasta_index: upload_fasta_device for the bytes of a FASTQ file.  Nothing is
        copied or compacted: the reads are packed out of buf itself, where each is one contiguous sequence line.
        more=True (mtr_upload_fastq_device_window): buf is the beginning of a longer input, as in parse_fastq_device.
        keep_quality=True (mtr_keep_qualities, for this call): the reads' quality lines stay with the batch as Phred values, for
        genotype_window_qualities; any later upload replaces or drops them."""
        if not keep_quality:
            return self._upload_file_device("mtr_upload_fastq_device", buf, file_state, more)
        self._check(self.lib.mtr_keep_qualities(self.h, 1), "mtr_keep_qualities")
        try:
            return self._upload_file_device("mtr_upload_fastq_device", buf, file_state, more)
        finally:
            self.lib.mtr_keep_qualities(self.h, 0)

    def qualities_resident(self) -> int:
        """mtr_qualities_resident: the Phred values kept with the resident batch, 0 when there are none"""
        nb = C.c_int64()
        self._check(self.lib.mtr_qualities_resident(self.h, C.byref(nb)), "mtr_qualities_resident")
        return int(nb.value)

    def attach_qualities(self, qual, offsets) -> None:
        """mtr_attach_qualities_device: Phred values (not ASCII) for the resident batch, whatever uploaded it - upload_device for one.  qual: a
        1-D uint8 tensor on this engine's device; offsets: per read of the batch where its values begin in qual (a host sequence of integers);
        read i's values are qual[offsets[i]:offsets[i] + lens[i]].  Values above 93 are stored as 93."""
        import torch

        if not isinstance(qual, torch.Tensor) or qual.dim() != 1:
            raise MtrError("qual must be a 1-D torch tensor")
        ptr = self._gpu_column(qual, torch.uint8, (int(qual.numel()),), "qual")
        offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        if len(offs) != self.n_reads:
            raise MtrError(f"{len(offs)} offsets for the resident batch of {self.n_reads} reads")
        stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        self._check(self.lib.mtr_attach_qualities_device(self.h, ptr, int(qual.numel()), offs.ctypes.data, stream), "mtr_attach_qualities_device")

    def _upload_file_device(self, entry: str, buf, file_state, more: bool = False) -> Fasta:
        import torch

        fasta_input_args(buf, self.device)
        stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        info = CFastaInfo()
        self.n_reads = 0
        src = C.c_void_p(buf.data_ptr()) if buf.numel() else None
        if more:
            self._check(getattr(self.lib, entry + "_window")(self.h, file_state.h if file_state is not None else None, src, buf.numel(), 1, stream,
                                                             C.byref(info)), entry + "_window")
        elif file_state is None:
            self._check(getattr(self.lib, entry)(self.h, src, buf.numel(), stream, C.byref(info)), entry)
        else:
            self._check(getattr(self.lib, entry + "_in_file")(self.h, file_state.h, src, buf.numel(), stream, C.byref(info)), entry + "_in_file")
        n = info.n_reads
        lens, id_off, ids = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(max(int(info.id_bytes), 1), np.uint8)
        self._check(self.lib.mtr_fasta_index(self.h, lens.ctypes.data, id_off.ctypes.data, ids.ctypes.data), "mtr_fasta_index")
        offsets = np.zeros(n, np.int64)
        if n > 1:
            offsets[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        self.n_reads = n
        return _fasta(info, None, offsets, lens, id_off, ids.tobytes()[:int(info.id_bytes)])

    def walk_fasta_device(self, buf, window_bytes: int, file_state: "FileState | None" = None):
        """A FASTA file on the GPU batch by batch: a generator over upload_fasta_device(buf[pos:pos + w], file_state, more), where
        w starts as window_bytes and more = pos + w < len(buf).  The slices are views: nothing is copied, and a window may start at
        any byte.  Yields one Fasta per call that uploaded reads - its reads are the resident batch: the caller runs and reports
        before taking the next item - and one last item whose end is not "more": the end of the whole file, with end_pos and
        bad_char as one upload_fasta_device(buf) would give them (end_pos of every item is absolute in buf).  That last item may
        have no reads; then nothing is resident and there is nothing to run.  A window smaller than its first record (no reads,
        "more") doubles w for the rest of the walk and is retried at the same pos; w is cut to what is left of buf, so the walk
        ends.  The reads of all items together are those of upload_fasta_device(buf), whatever window_bytes: a window ends on
        the header of its open record, which starts an fgets window of the reference's reader, so the next window is read as the
        whole file would be.  window_bytes < 1 raises MtrError before the library is called.
        Only a window is limited to INT32_MAX bytes: a buf of any length can be walked.  The loop of a C caller:
            pos = 0;
            do { n = min(w, len - pos);
                 mtr_upload_fasta_device_window(ctx, fs, d + pos, n, pos + n < len, stream, &info);
                 if (info.end == MTR_FASTA_END_MORE && info.n_reads == 0) { w *= 2; continue; }
                 if (info.n_reads > 0) { run; report; }
                 pos += info.end_pos;
            } while (info.end == MTR_FASTA_END_MORE);"""
        return self._walk_file_device(self.upload_fasta_device, buf, window_bytes, file_state)

    def walk_fastq_device(self, buf, window_bytes: int, file_state: "FileState | None" = None, keep_quality: bool = False):
        """walk_fasta_device for the bytes of a FASTQ file (upload_fastq_device, mtr_upload_fastq_device_window): a window's reads
        are the records whose quality line's LF lies in it, and the next window starts behind the last such LF.  keep_quality: as
        upload_fastq_device's, for every batch of the walk."""
        if not keep_quality:
            return self._walk_file_device(self.upload_fastq_device, buf, window_bytes, file_state)
        return self._walk_file_device(lambda part, fs, more: self.upload_fastq_device(part, fs, more, keep_quality=True), buf, window_bytes, file_state)

    def _walk_file_device(self, upload, buf, window_bytes, file_state):
        if isinstance(window_bytes, bool) or not isinstance(window_bytes, (int, np.integer)) or window_bytes < 1:
            raise MtrError(f"window_bytes must be an integer of at least 1, got {window_bytes!r}")
        fasta_input_args(buf, self.device)
        return self._walk(upload, buf, int(window_bytes), file_state)

    @staticmethod
    def _walk(upload, buf, w, file_state):
        n, pos = buf.numel(), 0
        while True:
            k = min(w, n - pos)
            f = upload(buf[pos:pos + k], file_state, pos + k < n)
            if f.end == "more" and len(f.lens) == 0:
                w *= 2
                continue
            yield f._replace(end_pos=pos + f.end_pos)
            if f.end != "more":
                return
            pos += f.end_pos

    def process_device(self, text, offsets, lens, codes: bool = False, file_state: "FileState | None" = None) -> List[List[Record]]:
        """upload_device + run + fetch: per read its records in insertion order, as process() (file_state: process_in_file()) returns them"""
        self.upload_device(text, offsets, lens, codes, file_state)
        self.run()
        return self.fetch()

    def export_tensor(self):
        """The wire-form record table of the last run (mtr_export_packed_device) in a fresh torch.uint8 tensor on this engine's
        device, and the records per read: returns (blob, counts int32 CPU tensor)."""
        import torch

        counts = np.zeros(self.n_reads, np.int32)
        total, nbytes = C.c_int64(), C.c_int64()
        st = self.lib.mtr_export_packed_device(self.h, None, 0, counts.ctypes.data, C.byref(total), C.byref(nbytes))   # capacity 0: the size
        if st not in (0, 5):                                                                                      # (MTR_ERR_OVERFLOW: size known)
            self._check(st, "mtr_export_packed_device")
        dev = torch.device("cuda", self.device)
        blob = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()            # the library writes blob on its own stream: torch's earlier use of the memory is done
        if nbytes.value:
            self._check(self.lib.mtr_export_packed_device(self.h, C.c_void_p(blob.data_ptr()), blob.numel(), counts.ctypes.data, C.byref(total),
                                                          C.byref(nbytes)), "mtr_export_packed_device")
        return blob[:int(nbytes.value)], torch.from_numpy(counts)

    def report_tensors(self) -> Report:
        """mTR's report of the last run (mtr_report_device), chained on the device: a Report of fresh tensors on this engine's device
        (counts on the CPU).  Follows export_tensor's stream handling."""
        import torch

        n = getattr(self, "n_reads", 0)                          # (nothing uploaded yet: the library answers MTR_ERR_BAD_ARG)
        counts = np.zeros(max(n, 1), np.int32)
        nrep, nub = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_report_device(self.h, None, counts.ctypes.data, C.byref(nrep), C.byref(nub)), "mtr_report_device")
        R, U = int(nrep.value), int(nub.value)
        dev = torch.device("cuda", self.device)
        read = torch.empty(R, dtype=torch.int32, device=dev)
        record = torch.empty(R, dtype=torch.int32, device=dev)
        fields = torch.empty((R, 14), dtype=torch.int32, device=dev)
        ratio = torch.empty(R, dtype=torch.float32, device=dev)
        unit_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
        units = torch.empty(U, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        ptr = lambda t: t.data_ptr() if t.numel() else None     # noqa: E731
        dst = CReportDst(ptr(read), ptr(record), ptr(fields), ptr(ratio), unit_off.data_ptr(), ptr(units), R, U)
        self._check(self.lib.mtr_report_device(self.h, C.byref(dst), counts.ctypes.data, C.byref(nrep), C.byref(nub)), "mtr_report_device")
        return Report(torch.from_numpy(counts[:n]), read, record, fields, ratio, unit_off, units)

    def report_alignment_tensors(self) -> ReportAlignments:
        """The -a alignments of report_tensors()' repeats (mtr_report_alignments_device), aligned and rendered on the device: a
        ReportAlignments of fresh tensors on this engine's device.  Follows report_tensors' stream handling."""
        import torch

        nrep, ncol = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_report_alignments_device(self.h, None, C.byref(nrep), C.byref(ncol)), "mtr_report_alignments_device")
        R, Cn = int(nrep.value), int(ncol.value)
        dev = torch.device("cuda", self.device)
        col_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
        ops = torch.empty(Cn, dtype=torch.uint8, device=dev)
        text = torch.empty((3, Cn), dtype=torch.uint8, device=dev)
        first = torch.empty((R, 2), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        ptr = lambda t: t.data_ptr() if t.numel() else None     # noqa: E731
        dst = CReportAlignDst(col_off.data_ptr(), ptr(ops), ptr(text), ptr(first), R, Cn)
        self._check(self.lib.mtr_report_alignments_device(self.h, C.byref(dst), C.byref(nrep), C.byref(ncol)), "mtr_report_alignments_device")
        return ReportAlignments(col_off, ops, text, first)

    def report_text(self, ids, alignments: bool = False) -> ReportText:
        """mTR's stdout for the last run (mtr_report_text_device), formatted on the device: the report lines, with alignments=True
        mTR -a's alignment blocks behind them - byte for byte format_report's result, as a ReportText of fresh tensors on this
        engine's device.  ids: one str or bytes per uploaded read.  Follows report_tensors' stream handling."""
        import torch

        n = getattr(self, "n_reads", 0)                          # (nothing uploaded yet: the library answers MTR_ERR_BAD_ARG)
        data, off = pack_ids(ids, n)
        mode = 1 if alignments else 0
        nb = C.c_int64()
        self._check(self.lib.mtr_report_text_device(self.h, data.ctypes.data, off.ctypes.data, mode, None, C.byref(nb)), "mtr_report_text_device")
        B = int(nb.value)
        dev = torch.device("cuda", self.device)
        text = torch.empty(B, dtype=torch.uint8, device=dev)
        read_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()            # the library writes the tensors on its own stream: torch's earlier use of the memory is done
        dst = CReportTextDst(text.data_ptr() if B else None, read_off.data_ptr(), B)
        self._check(self.lib.mtr_report_text_device(self.h, data.ctypes.data, off.ctypes.data, mode, C.byref(dst), C.byref(nb)), "mtr_report_text_device")
        return ReportText(text, read_off)

    def report_bytes(self, ids, alignments: bool = False) -> bytes:
        """report_text(ids, alignments).text on the host: one device-to-host copy of the finished text"""
        return self.report_text(ids, alignments).text.cpu().numpy().tobytes()

    def report_motif_tensors(self) -> ReportMotifs:
        """The motif catalogue of report_tensors()' repeats (mtr_report_motifs_device), made on the device: a ReportMotifs of fresh tensors
        on this engine's device.  Follows report_tensors' stream handling."""
        import torch

        nrep, ngrp, nmb = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_report_motifs_device(self.h, None, C.byref(nrep), C.byref(ngrp), C.byref(nmb)), "mtr_report_motifs_device")
        R, G, M = int(nrep.value), int(ngrp.value), int(nmb.value)
        dev = torch.device("cuda", self.device)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)     # noqa: E731
        i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)     # noqa: E731
        u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)      # noqa: E731
        mot = ReportMotifs(u8(R), i32(R), i32(R), i32(R), i64(G + 1), u8(M), i32(G), i32(G), i32(G), i64(G), i64(G))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        ptr = lambda t: t.data_ptr() if t.numel() else None     # noqa: E731
        dst = CReportMotifDst(*[ptr(t) for t in mot], R, G, M)
        self._check(self.lib.mtr_report_motifs_device(self.h, C.byref(dst), C.byref(nrep), C.byref(ngrp), C.byref(nmb)), "mtr_report_motifs_device")
        return mot

    def search_motifs(self, motifs, gain: int = 1, mismatch: int = 1, indel: int = 1, both_strands: bool = True) -> MotifHits:
        """Known-motif search (mtr_search_motifs_device): every motif - a sequence of str or bytes over upper-case ACGT, 1..499 bases each -
        aligned to every read of the uploaded batch by the wrap-around DP with the given scores, on both strands unless both_strands is false.
        Needs no run and changes nothing a run left.  Returns a MotifHits of fresh tensors on this engine's device; follows report_tensors'
        stream handling."""
        import torch

        if isinstance(motifs, (str, bytes, bytearray)) or not hasattr(motifs, "__len__"):
            raise MtrError(f"motifs must be a sequence of str or bytes, got {type(motifs).__name__}")
        data, off = pack_ids(motifs)
        m = len(motifs)
        args = (self.h, data.ctypes.data, off.ctypes.data, m, int(gain), int(mismatch), int(indel), 1 if both_strands else 0)
        nh = C.c_int64()
        self._check(self.lib.mtr_search_motifs_device(*args, None, C.byref(nh)), "mtr_search_motifs_device")
        H = int(nh.value)
        n = H // m
        dev = torch.device("cuda", self.device)
        hits = MotifHits(torch.empty((n, m, 8), dtype=torch.int32, device=dev), torch.empty((n, m), dtype=torch.int32, device=dev),
                         torch.empty((n, m), dtype=torch.float32, device=dev), torch.empty((n, m), dtype=torch.uint8, device=dev))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CMotifHitsDst(*[t.data_ptr() for t in hits], H)
        self._check(self.lib.mtr_search_motifs_device(*args, C.byref(dst), C.byref(nh)), "mtr_search_motifs_device")
        return hits

    def search_motif_loci(self, motifs, min_score: int, gain: int = 1, mismatch: int = 1, indel: int = 1, both_strands: bool = True,
                          max_rounds: int = 16) -> MotifLoci:
        """Known-motif locus search (mtr_search_motif_loci_device, mtr_motif_loci_copy_device): EVERY place of every motif in every read of the
        uploaded batch whose alignment scores at least min_score, not only the best one of search_motifs - what lies left and right of a hit
        is aligned again, at most max_rounds (1..32) levels deep; `open` marks the pairs where that bound ended the search.  Needs no run and
        changes nothing a run left.  Returns a MotifLoci of fresh tensors on this engine's device; follows search_motifs' stream handling."""
        import torch

        if isinstance(motifs, (str, bytes, bytearray)) or not hasattr(motifs, "__len__"):
            raise MtrError(f"motifs must be a sequence of str or bytes, got {type(motifs).__name__}")
        data, off = pack_ids(motifs)
        m = len(motifs)
        npairs, nloci = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_search_motif_loci_device(self.h, data.ctypes.data, off.ctypes.data, m, int(gain), int(mismatch), int(indel),
                                                          1 if both_strands else 0, int(min_score), int(max_rounds), C.byref(npairs), C.byref(nloci)),
                    "mtr_search_motif_loci_device")
        Pn, T = int(npairs.value), int(nloci.value)
        n = Pn // m
        dev = torch.device("cuda", self.device)
        loci = MotifLoci(torch.empty((Pn + 1,), dtype=torch.int64, device=dev), torch.empty((T, 8), dtype=torch.int32, device=dev),
                         torch.empty((T,), dtype=torch.int32, device=dev), torch.empty((T,), dtype=torch.float32, device=dev),
                         torch.empty((T,), dtype=torch.uint8, device=dev), torch.empty((n, m), dtype=torch.uint8, device=dev))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CMotifLociDst(*[t.data_ptr() if t.numel() else None for t in loci], Pn, T)
        self._check(self.lib.mtr_motif_loci_copy_device(self.h, C.byref(dst)), "mtr_motif_loci_copy_device")
        return loci

    def search_flanks(self, patterns, both_strands: bool = True) -> FlankHits:
        """Flank search (mtr_search_flanks_device): every pattern - a sequence of str or bytes over upper-case ACGT, 1..64 bases each - matched
        approximately (unit-cost edit distance) against every read of the uploaded batch, on both strands unless both_strands is false: the
        nearest substring of the read, the leftmost end and then the shortest on ties.  Needs no run and changes nothing a run left.  Returns
        a FlankHits of fresh tensors on this engine's device; follows search_motifs' stream handling."""
        import torch

        if isinstance(patterns, (str, bytes, bytearray)) or not hasattr(patterns, "__len__"):
            raise MtrError(f"patterns must be a sequence of str or bytes, got {type(patterns).__name__}")
        data, off = pack_ids(patterns)
        m = len(patterns)
        args = (self.h, data.ctypes.data, off.ctypes.data, m, 1 if both_strands else 0)
        nh = C.c_int64()
        self._check(self.lib.mtr_search_flanks_device(*args, None, C.byref(nh)), "mtr_search_flanks_device")
        H = int(nh.value)
        n = H // m
        dev = torch.device("cuda", self.device)
        hits = FlankHits(*[torch.empty((n, m), dtype=torch.int32, device=dev) for _ in range(3)], torch.empty((n, m), dtype=torch.uint8, device=dev))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CFlankHitsDst(*[t.data_ptr() for t in hits], H)
        self._check(self.lib.mtr_search_flanks_device(*args, C.byref(dst), C.byref(nh)), "mtr_search_flanks_device")
        return hits

    def genotype_loci(self, loci, max_flank_dist: int, gain: int = 1, mismatch: int = 1, indel: int = 1) -> Genotypes:
        """Locus genotyping (mtr_genotype_loci_device): loci is a sequence of (left_flank, motif, right_flank), each str or bytes over upper-case
        ACGT - flanks of 1..64 bases, a motif of 1..499.  A read spans a locus where both flanks are found within max_flank_dist edits and in
        order, on either strand; the bases between them are aligned to the motif by search_motifs' DP with the given scores.  Needs no run and
        changes nothing a run left.  Returns a Genotypes of fresh tensors on this engine's device; follows search_motifs' stream handling."""
        import torch

        if isinstance(loci, (str, bytes, bytearray)) or not hasattr(loci, "__len__"):
            raise MtrError(f"loci must be a sequence of (left_flank, motif, right_flank), got {type(loci).__name__}")
        flat = []
        for k, locus in enumerate(loci):
            if isinstance(locus, (str, bytes, bytearray)) or not hasattr(locus, "__len__") or len(locus) != 3:
                raise MtrError(f"locus {k} must be (left_flank, motif, right_flank)")
            flat.extend(locus)
        data, off = pack_ids(flat)
        m = len(loci)
        args = (self.h, data.ctypes.data, off.ctypes.data, m, int(max_flank_dist), int(gain), int(mismatch), int(indel))
        nr = C.c_int64()
        self._check(self.lib.mtr_genotype_loci_device(*args, None, C.byref(nr)), "mtr_genotype_loci_device")
        R = int(nr.value)
        n = R // m
        dev = torch.device("cuda", self.device)
        new = lambda dtype, *tail: torch.empty((n, m) + tail, dtype=dtype, device=dev)     # noqa: E731
        gt = Genotypes(new(torch.uint8), new(torch.uint8), new(torch.int32, 2), new(torch.int32, 2), new(torch.int32, 8), new(torch.int32), new(torch.float32))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CGenotypesDst(*[t.data_ptr() for t in gt], R)
        self._check(self.lib.mtr_genotype_loci_device(*args, C.byref(dst), C.byref(nr)), "mtr_genotype_loci_device")
        return gt

    def genotype_catalog(self, loci, max_flank_dist: int, seed_len: "int | None" = None, gain: int = 1, mismatch: int = 1, indel: int = 1) -> SparseGenotypes:
        """Catalogue genotype (mtr_genotype_catalog_device, mtr_genotype_catalog_copy_device): loci and scores as genotype_loci takes them, any
        number of loci.  Returns the rows genotype_loci would mark spanning, bit for bit, as a SparseGenotypes sorted by (read, locus): a read
        is compared with a locus only where it holds an exact seed_len-mer of both flanks (exact: max_flank_dist edits cannot touch all of a
        flank's max_flank_dist + 1 disjoint seeds), so every flank needs (max_flank_dist + 1) * seed_len bases, 8 <= seed_len <= 16.
        seed_len = None picks the largest the flanks admit.  Needs no run and changes nothing a run left; follows genotype_loci's stream
        handling."""
        import torch

        data, off, m, seed_len = catalog_loci_args(loci, max_flank_dist, seed_len)
        nr, nc = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_genotype_catalog_device(self.h, data.ctypes.data, off.ctypes.data, m, int(max_flank_dist), int(seed_len), int(gain), int(mismatch),
                                                         int(indel), C.byref(nr), C.byref(nc)), "mtr_genotype_catalog_device")
        return self._catalog_rows(m, int(nr.value), int(nc.value))

    def _catalog_rows(self, m: int, R: int, candidates: int) -> SparseGenotypes:
        """the R rows a catalogue genotype call kept in the context, as fresh tensors (mtr_genotype_catalog_copy_device)"""
        import torch

        dev = torch.device("cuda", self.device)
        new = lambda dtype, *tail: torch.empty((R,) + tail, dtype=dtype, device=dev)     # noqa: E731
        cols = (new(torch.int32), new(torch.int32), new(torch.uint8), new(torch.uint8), new(torch.int32, 2), new(torch.int32, 2), new(torch.int32, 8), new(torch.int32),
                new(torch.float32))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CCatalogDst(cols[0].data_ptr(), cols[1].data_ptr(), CGenotypesDst(*[t.data_ptr() for t in cols[2:]], R))
        self._check(self.lib.mtr_genotype_catalog_copy_device(self.h, C.byref(dst)), "mtr_genotype_catalog_copy_device")
        return SparseGenotypes(self.n_reads, m, *cols, candidates)

    def build_catalog(self, loci, max_flank_dist: int, seed_len: "int | None" = None) -> Catalog:
        """A prepared catalogue (mtr_catalog_create): loci, max_flank_dist and seed_len as genotype_catalog takes them, with its checks and its
        choice of seed_len.  loci may also be the sequences already packed as the C call takes them - (uint8 array, int64 offsets with
        3 * n_loci + 1 entries: left flank, motif, right flank per locus) - which skips the string packing; seed_len is then required.  Built on
        this engine's device from one upload of the letters; needs no uploaded batch and changes nothing a batch or a run left.  The result
        is for genotype_prepared / genotype_partial_prepared of any Engine on this device, batch after batch."""
        if isinstance(loci, tuple) and len(loci) == 2 and isinstance(loci[0], np.ndarray) and isinstance(loci[1], np.ndarray):
            data, off = np.ascontiguousarray(loci[0], dtype=np.uint8), np.ascontiguousarray(loci[1], dtype=np.int64)
            if len(off) < 4 or (len(off) - 1) % 3 != 0:
                raise MtrError(f"packed loci need 3 * n_loci + 1 offsets, got {len(off)}")
            if seed_len is None:
                raise MtrError("packed loci need a seed_len")
            if int(off[0]) < 0 or int(off[-1]) > len(data):
                raise MtrError(f"the offsets reach {int(off[-1])}, the sequences hold {len(data)} bytes")
            m = (len(off) - 1) // 3
        else:
            data, off, m, seed_len = catalog_loci_args(loci, max_flank_dist, seed_len)
        h = C.c_void_p()
        self._check(self.lib.mtr_catalog_create(self.h, data.ctypes.data, off.ctypes.data, m, int(max_flank_dist), int(seed_len), C.byref(h)), "mtr_catalog_create")
        return Catalog(self.lib, h, self.device)

    def genotype_prepared(self, cat: Catalog, gain: int = 1, mismatch: int = 1, indel: int = 1) -> SparseGenotypes:
        """genotype_catalog on a prepared catalogue (mtr_genotype_catalog_prepared_device): the same SparseGenotypes, bit for bit, as
        genotype_catalog returns for the catalogue's loci, max_flank_dist and seed_len on the resident batch, without rebuilding anything that
        depends on the loci alone."""
        nr, nc = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_genotype_catalog_prepared_device(self.h, cat._handle(), int(gain), int(mismatch), int(indel), C.byref(nr), C.byref(nc)),
                    "mtr_genotype_catalog_prepared_device")
        return self._catalog_rows(cat.n_loci, int(nr.value), int(nc.value))

    def genotype_partial_prepared(self, cat: Catalog, gain: int = 1, mismatch: int = 1, indel: int = 1, max_tail: int = 10) -> SparsePartialGenotypes:
        """genotype_partial_catalog on a prepared catalogue (mtr_genotype_partial_catalog_prepared_device): the same SparsePartialGenotypes, bit
        for bit; a catalogue with a motif of more than 32 bases is refused as genotype_partial_catalog refuses such loci."""
        nr, nc = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_genotype_partial_catalog_prepared_device(self.h, cat._handle(), int(gain), int(mismatch), int(indel), int(max_tail), C.byref(nr),
                                                                          C.byref(nc)), "mtr_genotype_partial_catalog_prepared_device")
        return self._partial_catalog_rows(cat.n_loci, int(nr.value), int(nc.value))

    def genotype_partial(self, loci, max_flank_dist: int, gain: int = 1, mismatch: int = 1, indel: int = 1, max_tail: int = 10) -> PartialGenotypes:
        """Partial genotype (mtr_genotype_partial_device): loci as genotype_loci takes them, motifs of at most 32 bases.  A read that does not
        span a locus but holds one of its flanks within max_flank_dist edits is extended from that flank towards the read's end by the anchored
        wrap-around DP with the given scores; where the extension ends within max_tail bases of the read's end the row is open: its copies are a
        lower bound.  Needs no run and changes nothing a run left.  Returns a PartialGenotypes of fresh tensors on this engine's device; follows
        genotype_loci's stream handling."""
        import torch

        if isinstance(loci, (str, bytes, bytearray)) or not hasattr(loci, "__len__"):
            raise MtrError(f"loci must be a sequence of (left_flank, motif, right_flank), got {type(loci).__name__}")
        flat = []
        for k, locus in enumerate(loci):
            if isinstance(locus, (str, bytes, bytearray)) or not hasattr(locus, "__len__") or len(locus) != 3:
                raise MtrError(f"locus {k} must be (left_flank, motif, right_flank)")
            flat.extend(locus)
        data, off = pack_ids(flat)
        m = len(loci)
        args = (self.h, data.ctypes.data, off.ctypes.data, m, int(max_flank_dist), int(gain), int(mismatch), int(indel), int(max_tail))
        nr = C.c_int64()
        self._check(self.lib.mtr_genotype_partial_device(*args, None, C.byref(nr)), "mtr_genotype_partial_device")
        R = int(nr.value)
        n = R // m
        dev = torch.device("cuda", self.device)
        new = lambda dtype, *tail: torch.empty((n, m) + tail, dtype=dtype, device=dev)     # noqa: E731
        pg = PartialGenotypes(new(torch.uint8), new(torch.uint8), new(torch.int32), new(torch.int32, 2), new(torch.int32, 6), new(torch.float32), new(torch.uint8))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CPartialDst(*[t.data_ptr() for t in pg], R)
        self._check(self.lib.mtr_genotype_partial_device(*args, C.byref(dst), C.byref(nr)), "mtr_genotype_partial_device")
        return pg

    def genotype_partial_catalog(self, loci, max_flank_dist: int, seed_len: "int | None" = None, gain: int = 1, mismatch: int = 1, indel: int = 1,
                                 max_tail: int = 10) -> SparsePartialGenotypes:
        """Partial genotype at catalogue scale (mtr_genotype_partial_catalog_device, mtr_genotype_partial_catalog_copy_device): loci, scores and
        max_tail as genotype_partial takes them, any number of loci.  Returns the rows genotype_partial would mark partial, bit for bit, as a
        SparsePartialGenotypes sorted by (read, locus): a read is compared with a locus only where it holds an exact seed_len-mer of at least
        one of its four flank patterns (exact: max_flank_dist edits cannot touch all of a flank's max_flank_dist + 1 disjoint seeds), and only
        the seeded patterns are scanned; every flank needs (max_flank_dist + 1) * seed_len bases, 8 <= seed_len <= 16.  seed_len = None picks
        the largest the flanks admit.  Needs no run and changes nothing a run or genotype_catalog left; follows genotype_loci's stream handling."""
        import torch

        data, off, m, seed_len = catalog_loci_args(loci, max_flank_dist, seed_len)
        nr, nc = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_genotype_partial_catalog_device(self.h, data.ctypes.data, off.ctypes.data, m, int(max_flank_dist), int(seed_len), int(gain), int(mismatch),
                                                                 int(indel), int(max_tail), C.byref(nr), C.byref(nc)), "mtr_genotype_partial_catalog_device")
        return self._partial_catalog_rows(m, int(nr.value), int(nc.value))

    def _partial_catalog_rows(self, m: int, R: int, candidates: int) -> SparsePartialGenotypes:
        """the R rows a partial catalogue call kept in the context, as fresh tensors (mtr_genotype_partial_catalog_copy_device)"""
        import torch

        dev = torch.device("cuda", self.device)
        new = lambda dtype, *tail: torch.empty((R,) + tail, dtype=dtype, device=dev)     # noqa: E731
        cols = (new(torch.int32), new(torch.int32), new(torch.uint8), new(torch.uint8), new(torch.int32), new(torch.int32, 2), new(torch.int32, 6), new(torch.float32),
                new(torch.uint8))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CPartialCatalogDst(cols[0].data_ptr(), cols[1].data_ptr(), CPartialDst(*[t.data_ptr() for t in cols[2:]], R))
        self._check(self.lib.mtr_genotype_partial_catalog_copy_device(self.h, C.byref(dst)), "mtr_genotype_partial_catalog_copy_device")
        return SparsePartialGenotypes(self.n_reads, m, *cols, candidates)

    def call_alleles(self, gt, measure="copies", min_ratio: float = 0.0, min_support: int = 2, min_percent: int = 20, min_sep: int = 1) -> AlleleCalls:
        """Allele calls (mtr_call_alleles_device): the rows of genotype_loci - one call's Genotypes, or several batches' joined with torch.cat(dim=0)
        column by column - reduced per locus.  gt may also be a SparseGenotypes (mtr_call_alleles_rows_device): genotype_catalog's result, or
        several batches' - SparseGenotypes(n_reads summed, n_loci, then every column joined with torch.cat after the batch's first read's index
        was added to its `read`) - with the same calls as the dense rows give; no (read, locus) may occur twice.  A row supports its locus when it spans it and its ratio is at least min_ratio (a row with an empty
        window always does); its value is its copies (measure "copies" / ALLELE_COPIES) or its window's bases ("bases" / ALLELE_BASES).  Per locus
        the supporting reads are sorted by (value, read) and split into two alleles where a split exists whose smaller side has min_support reads
        and min_percent percent of them and whose medians lie min_sep apart - the split of least absolute deviation from the two medians.  Needs no
        upload and no run and changes nothing either left.  Returns an AlleleCalls of fresh tensors on this engine's device; waits for torch's
        current stream (where gt was written) by an event, and follows genotype_loci's stream handling for its results."""
        import torch

        if isinstance(measure, str) and measure in ("copies", "bases"):
            code = ALLELE_COPIES if measure == "copies" else ALLELE_BASES
        elif isinstance(measure, (int, np.integer)) and not isinstance(measure, bool) and int(measure) in (ALLELE_COPIES, ALLELE_BASES):
            code = int(measure)
        else:
            raise MtrError(f"measure must be 'copies', 'bases', ALLELE_COPIES or ALLELE_BASES, got {measure!r}")
        dev = torch.device("cuda", self.device)
        prm = CAlleleParams(code, float(min_ratio), int(min_support), int(min_percent), int(min_sep))
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if isinstance(gt, SparseGenotypes):
            R, m = sparse_rows_args(gt, self.device)
            ptr = lambda t: t.data_ptr() if R else None     # noqa: E731
            rows = CGenotypesDst(ptr(gt.spanning), None, None, ptr(gt.window), ptr(gt.fields), None, ptr(gt.ratio), R)
            call, name = self.lib.mtr_call_alleles_rows_device, "mtr_call_alleles_rows_device"
            args = (self.h, C.byref(rows), ptr(gt.read), ptr(gt.locus), R, m, C.byref(prm), stream)
        else:
            n, m = genotype_rows_args(gt, self.device)
            rows = CGenotypesDst(gt.spanning.data_ptr(), None, None, gt.window.data_ptr(), gt.fields.data_ptr(), None, gt.ratio.data_ptr(), n * m)
            call, name = self.lib.mtr_call_alleles_device, "mtr_call_alleles_device"
            args = (self.h, C.byref(rows), n, m, C.byref(prm), stream)
        ns = C.c_int64()
        self._check(call(*args, None, C.byref(ns)), name)
        S = int(ns.value)
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)     # noqa: E731
        calls = AlleleCalls(new(torch.int64, m + 1), new(torch.int32, S), new(torch.int32, S), new(torch.uint8, S), new(torch.uint8, m),
                            new(torch.int32, m, 2), new(torch.int32, m, 2), new(torch.int64, m, 2))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CAlleleCallsDst(*[t.data_ptr() if t.numel() else None for t in calls], m, S)
        self._check(call(*args, C.byref(dst), C.byref(ns)), name)
        return calls

    def _gpu_column(self, t, dtype, shape, what: str):
        import torch

        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise MtrError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)}")
        if not t.is_cuda or t.device.index != self.device:
            raise MtrError(f"{what} is on {t.device}, the engine on cuda:{self.device}")
        return t.data_ptr() if t.numel() else None

    def genotype_windows(self, sg) -> GenotypeWindows:
        """The oriented windows of a SparseGenotypes' rows out of the RESIDENT batch (mtr_extract_windows_device): call it on the batch's own
        result - genotype_catalog's or genotype_prepared's, or genotype_loci(...).to_sparse() - before the next upload and before
        join_sparse_genotypes adds an offset to `read`.  Row r's window is bases[off[r]:off[r + 1]], reverse-complemented where orientation is 1.
        Returns fresh tensors on this engine's device; stream handling as call_alleles'."""
        import torch

        R = int(sg.read.numel()) if isinstance(sg.read, torch.Tensor) and sg.read.dim() == 1 else -1
        if R < 0:
            raise MtrError("the rows' read column must be a 1-D torch tensor")
        ptrs = [self._gpu_column(sg.read, torch.int32, (R,), "the rows' read"), self._gpu_column(sg.orientation, torch.uint8, (R,), "the rows' orientation"),
                self._gpu_column(sg.window, torch.int32, (R, 2), "the rows' window")]
        dev = torch.device("cuda", self.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nb = C.c_int64()
        self._check(self.lib.mtr_extract_windows_device(self.h, *ptrs, R, stream, None, C.byref(nb)), "mtr_extract_windows_device")
        T = int(nb.value)
        win = GenotypeWindows(torch.empty(R + 1, dtype=torch.int64, device=dev), torch.empty(T, dtype=torch.uint8, device=dev))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CWindowsDst(win.off.data_ptr(), win.bases.data_ptr() if T else None, R, T)
        self._check(self.lib.mtr_extract_windows_device(self.h, *ptrs, R, stream, C.byref(dst), C.byref(nb)), "mtr_extract_windows_device")
        return win

    def genotype_window_qualities(self, sg):
        """The Phred values of genotype_windows(sg)'s bases (mtr_extract_window_qualities_device): a uint8 tensor [T] aligned with its `bases`,
        row r's at off[r]:off[r + 1], reversed - not complemented - where orientation is 1.  Needs the batch's qualities: an upload with
        keep_quality=True, or attach_qualities.  Several batches' are joined by join_window_qualities."""
        import torch

        R = int(sg.read.numel()) if isinstance(sg.read, torch.Tensor) and sg.read.dim() == 1 else -1
        if R < 0:
            raise MtrError("the rows' read column must be a 1-D torch tensor")
        ptrs = [self._gpu_column(sg.read, torch.int32, (R,), "the rows' read"), self._gpu_column(sg.orientation, torch.uint8, (R,), "the rows' orientation"),
                self._gpu_column(sg.window, torch.int32, (R, 2), "the rows' window")]
        dev = torch.device("cuda", self.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nb = C.c_int64()
        call = self.lib.mtr_extract_window_qualities_device
        self._check(call(self.h, *ptrs, R, stream, None, 0, C.byref(nb)), "mtr_extract_window_qualities_device")
        T = int(nb.value)
        qual = torch.empty(T, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()            # the library writes the column on its own stream: torch's earlier use of the memory is done
        if T:
            self._check(call(self.h, *ptrs, R, stream, qual.data_ptr(), T, C.byref(nb)), "mtr_extract_window_qualities_device")
        return qual

    def allele_consensus_quality(self, sg, windows: GenotypeWindows, qual, calls: AlleleCalls, band_extra: int = 16, qual_cap: int = 40) -> AlleleConsensus:
        """Quality-weighted allele consensus (mtr_allele_consensus_quality_device): allele_consensus - the same backbone, alignments, skip rule
        and tie rules - with every vote weighted by its base's Phred value: a base of quality q weighs min(max(q, 1), qual_cap), a deletion or
        the end of an insertion the lighter of the two bases beside it.  qual: the windows' qualities (genotype_window_qualities, or
        join_window_qualities'), aligned with windows.bases.  `votes` holds weight sums; format_allele_consensus, window_structure and
        window_edits take the result as they take allele_consensus'.  qual_cap = 1 is allele_consensus."""
        import torch

        if isinstance(qual_cap, bool) or not isinstance(qual_cap, (int, np.integer)):
            raise MtrError(f"qual_cap must be an integer, got {qual_cap!r}")
        if not isinstance(qual, torch.Tensor) or qual.dim() != 1:
            raise MtrError("qual must be a 1-D torch tensor")
        return self._allele_consensus(sg, windows, calls, band_extra, (qual, int(qual_cap)))

    def allele_consensus(self, sg, windows: GenotypeWindows, calls: AlleleCalls, band_extra: int = 16) -> AlleleConsensus:
        """Allele consensus (mtr_allele_consensus_device): each called allele's sequence by vote.  sg: the SparseGenotypes the calls were made of
        (one batch's, or join_sparse_genotypes'), sorted by (read, locus); windows: its rows' windows (genotype_windows, or join_windows'); calls:
        call_alleles(sg, ...).  Per allele the member in the middle of its (value, read) order is the backbone; every other member is aligned to
        it by a banded edit distance (the band is |length difference| + 2 * band_extra + 1 diagonals wide; a member whose band exceeds 256 or
        whose window, or the backbone's, exceeds 16384 bases is counted as skipped) and votes per backbone position for a base, a deletion or up
        to four inserted bases; the consensus is the plurality, ties to the backbone.  Needs no upload and no run and changes nothing either
        left.  Returns an AlleleConsensus of fresh tensors on this engine's device; stream handling as call_alleles'."""
        return self._allele_consensus(sg, windows, calls, band_extra, None)

    def _allele_consensus(self, sg, windows, calls, band_extra, weights):
        """allele_consensus (weights None) and allele_consensus_quality (weights = (qual, qual_cap)): one argument list, one sizing call, one writing call"""
        import torch

        if isinstance(band_extra, bool) or not isinstance(band_extra, (int, np.integer)):
            raise MtrError(f"band_extra must be an integer, got {band_extra!r}")
        if isinstance(sg.n_loci, bool) or not isinstance(sg.n_loci, (int, np.integer)) or sg.n_loci < 1:
            raise MtrError(f"n_loci must be an integer >= 1, got {sg.n_loci!r}")
        if not isinstance(sg.read, torch.Tensor) or sg.read.dim() != 1 or not isinstance(calls.read, torch.Tensor) or calls.read.dim() != 1:
            raise MtrError("the rows' and the calls' read columns must be 1-D torch tensors")
        if not isinstance(windows.bases, torch.Tensor) or windows.bases.dim() != 1:
            raise MtrError("the windows' bases must be a 1-D torch tensor")
        R, S, T, m = int(sg.read.numel()), int(calls.read.numel()), int(windows.bases.numel()), int(sg.n_loci)
        col = self._gpu_column
        src = CConsensusSrc(col(sg.read, torch.int32, (R,), "the rows' read"), col(sg.locus, torch.int32, (R,), "the rows' locus"),
                            col(windows.off, torch.int64, (R + 1,), "the windows' off"), col(windows.bases, torch.uint8, (T,), "the windows' bases"),
                            col(calls.support_off, torch.int64, (m + 1,), "the calls' support_off"), col(calls.read, torch.int32, (S,), "the calls' read"),
                            col(calls.allele, torch.uint8, (S,), "the calls' allele"), col(calls.zygosity, torch.uint8, (m,), "the calls' zygosity"), R, T, S, m)
        dev = torch.device("cuda", self.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        nb = C.c_int64()
        if weights is None:
            entry = "mtr_allele_consensus_device"
            call = lambda s, extra, st, dst, out: self.lib.mtr_allele_consensus_device(self.h, s, extra, st, dst, out)      # noqa: E731
        else:
            entry = "mtr_allele_consensus_quality_device"
            q, cap = col(weights[0], torch.uint8, (T,), "qual"), weights[1]
            call = lambda s, extra, st, dst, out: self.lib.mtr_allele_consensus_quality_device(self.h, s, q, extra, cap, st, dst, out)      # noqa: E731
        self._check(call(C.byref(src), int(band_extra), stream, None, C.byref(nb)), entry)
        L = int(nb.value)
        new = lambda dtype, n: torch.empty(n, dtype=dtype, device=dev)     # noqa: E731
        cons = AlleleConsensus(new(torch.int64, 2 * m + 1), new(torch.uint8, L), new(torch.int32, L), *[new(torch.int32, 2 * m) for _ in range(5)])
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CConsensusDst(*[t.data_ptr() if t.numel() else None for t in cons], 2 * m, L)
        self._check(call(C.byref(src), int(band_extra), stream, C.byref(dst), C.byref(nb)), entry)
        return cons

    def call_alleles_by_sequence(self, sg, windows: GenotypeWindows, calls: AlleleCalls, max_dist: int = 32, min_support: int = 2, min_percent: int = 20,
                                 min_sep: int = 1, min_gain: int = 0) -> "SequenceCalls":
        """Allele calls by sequence (mtr_call_alleles_sequence_device, mtr_call_alleles_sequence_copy_device).  sg, windows and calls are
        allele_consensus' arguments; of calls only the support lists are read (support_off, value, read): which reads support a locus, in
        which order.  Per locus the edit distance between every two supporting reads' oriented windows, saturated at max_dist + 1, and the
        exact one- or two-medoid split over those distances: two alleles where a pair of medoids exists whose smaller side has min_support
        reads and min_percent percent of them, whose medoids lie min_sep apart, and whose cost is at most (100 - min_gain) percent of one
        medoid's - the pair of least cost.  A locus of more than SEQ_MAX_MEMBERS supporting reads is marked skipped.  Returns a
        SequenceCalls of fresh tensors on this engine's device; .calls goes unchanged into allele_consensus, format_allele_calls and
        partial_support.  Needs no upload and no run and changes nothing either left.  Stream handling as allele_consensus'."""
        import torch

        for name, v in (("max_dist", max_dist), ("min_support", min_support), ("min_percent", min_percent), ("min_sep", min_sep), ("min_gain", min_gain)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise MtrError(f"{name} must be an integer, got {v!r}")
        if isinstance(sg.n_loci, bool) or not isinstance(sg.n_loci, (int, np.integer)) or sg.n_loci < 1:
            raise MtrError(f"n_loci must be an integer >= 1, got {sg.n_loci!r}")
        if not isinstance(sg.read, torch.Tensor) or sg.read.dim() != 1 or not isinstance(calls.read, torch.Tensor) or calls.read.dim() != 1:
            raise MtrError("the rows' and the calls' read columns must be 1-D torch tensors")
        if not isinstance(windows.bases, torch.Tensor) or windows.bases.dim() != 1:
            raise MtrError("the windows' bases must be a 1-D torch tensor")
        R, S, T, m = int(sg.read.numel()), int(calls.read.numel()), int(windows.bases.numel()), int(sg.n_loci)
        col = self._gpu_column
        src = CConsensusSrc(col(sg.read, torch.int32, (R,), "the rows' read"), col(sg.locus, torch.int32, (R,), "the rows' locus"),
                            col(windows.off, torch.int64, (R + 1,), "the windows' off"), col(windows.bases, torch.uint8, (T,), "the windows' bases"),
                            col(calls.support_off, torch.int64, (m + 1,), "the calls' support_off"), col(calls.read, torch.int32, (S,), "the calls' read"),
                            None, None, R, T, S, m)
        value = col(calls.value, torch.int32, (S,), "the calls' value")
        prm = CSeqParams(int(max_dist), int(min_support), int(min_percent), int(min_sep), int(min_gain))
        dev = torch.device("cuda", self.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ns, npairs = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_call_alleles_sequence_device(self.h, C.byref(src), value, C.byref(prm), stream, C.byref(ns), C.byref(npairs)),
                    "mtr_call_alleles_sequence_device")
        P = int(npairs.value)
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)     # noqa: E731
        ac = AlleleCalls(new(torch.int64, m + 1), new(torch.int32, S), new(torch.int32, S), new(torch.uint8, S), new(torch.uint8, m),
                         new(torch.int32, m, 2), new(torch.int32, m, 2), new(torch.int64, m, 2))
        sc = SequenceCalls(ac, new(torch.int32, m, 2), new(torch.int32, S), new(torch.uint8, m), new(torch.int64, m + 1), new(torch.uint8, P))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CSeqCallsDst(*[t.data_ptr() if t.numel() else None for t in (*ac, *sc[1:])], m, S, P)
        self._check(self.lib.mtr_call_alleles_sequence_copy_device(self.h, C.byref(dst)), "mtr_call_alleles_sequence_copy_device")
        return sc

    def genotype_quality(self, sg, windows: GenotypeWindows, qual, calls: AlleleCalls, cons: AlleleConsensus, band_extra: int = 16, qual_cap: int = 40,
                         gap_cap: int = 20, read_cap: int = 60) -> "GenotypeQuality":
        """Genotype quality (mtr_genotype_quality_device).  sg, windows and calls are allele_consensus' arguments, qual the windows' qualities
        (genotype_window_qualities; None: every base weighs qual_cap), cons the alleles' sequences (allele_consensus' or
        allele_consensus_quality's result over the same calls).  Every supporting read's window is aligned to both allele sequences of its
        locus inside the consensus' band with the read's qualities as costs - a substitution costs min(max(q, 1), qual_cap), a gap step at
        most gap_cap -; per read the better allele and the margin, per locus the sums of the scores (one read's capped at read_cap) for the
        genotypes 0/0, 0/1, 1/1, and from them pl, gt and gq as a VCF words them.  The defaults are policy, not measured on a basecaller's
        output.  Returns a GenotypeQuality of fresh tensors on this engine's device.  Needs no upload and no run and changes nothing either
        left.  Stream handling as allele_consensus'."""
        import torch

        for name, v in (("band_extra", band_extra), ("qual_cap", qual_cap), ("gap_cap", gap_cap), ("read_cap", read_cap)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise MtrError(f"{name} must be an integer, got {v!r}")
        if isinstance(sg.n_loci, bool) or not isinstance(sg.n_loci, (int, np.integer)) or sg.n_loci < 1:
            raise MtrError(f"n_loci must be an integer >= 1, got {sg.n_loci!r}")
        if not isinstance(sg.read, torch.Tensor) or sg.read.dim() != 1 or not isinstance(calls.read, torch.Tensor) or calls.read.dim() != 1:
            raise MtrError("the rows' and the calls' read columns must be 1-D torch tensors")
        if not isinstance(windows.bases, torch.Tensor) or windows.bases.dim() != 1 or not isinstance(cons.bases, torch.Tensor) or cons.bases.dim() != 1:
            raise MtrError("the windows' and the consensus' bases must be 1-D torch tensors")
        if qual is not None and (not isinstance(qual, torch.Tensor) or qual.dim() != 1):
            raise MtrError("qual must be a 1-D torch tensor or None")
        R, S, T, m, L = int(sg.read.numel()), int(calls.read.numel()), int(windows.bases.numel()), int(sg.n_loci), int(cons.bases.numel())
        col = self._gpu_column
        src = CConsensusSrc(col(sg.read, torch.int32, (R,), "the rows' read"), col(sg.locus, torch.int32, (R,), "the rows' locus"),
                            col(windows.off, torch.int64, (R + 1,), "the windows' off"), col(windows.bases, torch.uint8, (T,), "the windows' bases"),
                            col(calls.support_off, torch.int64, (m + 1,), "the calls' support_off"), col(calls.read, torch.int32, (S,), "the calls' read"),
                            col(calls.allele, torch.uint8, (S,), "the calls' allele"), col(calls.zygosity, torch.uint8, (m,), "the calls' zygosity"), R, T, S, m)
        q = None if qual is None else col(qual, torch.uint8, (T,), "qual")
        cons_off, cons_bases = col(cons.off, torch.int64, (2 * m + 1,), "the consensus' off"), col(cons.bases, torch.uint8, (L,), "the consensus' bases")
        prm = CGqParams(int(band_extra), int(qual_cap), int(gap_cap), int(read_cap))
        dev = torch.device("cuda", self.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)     # noqa: E731
        gq = GenotypeQuality(new(torch.int32, S, 2), new(torch.uint8, S), new(torch.int32, S), new(torch.int64, m, 3), new(torch.int64, m, 3), new(torch.uint8, m),
                             new(torch.int64, m), new(torch.int32, m), new(torch.int32, m))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CGqDst(*[t.data_ptr() if t.numel() else None for t in gq], S, m)
        self._check(self.lib.mtr_genotype_quality_device(self.h, C.byref(src), q, cons_off, cons_bases, L, C.byref(prm), stream, C.byref(dst)), "mtr_genotype_quality_device")
        return gq

    def _window_args(self, structures, off, bases, which, gain, mismatch, indel):
        """what window_structure and window_edits hand to the library for their common arguments, in the calls' order up to wait_stream: the
        host arrays of the structures (kept alive by the caller through the returned tuple), the device columns, N, T, the scores, the stream"""
        import torch

        for name, v in (("gain", gain), ("mismatch", mismatch), ("indel", indel)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise MtrError(f"{name} must be an integer, got {v!r}")
        lists = [[st] if isinstance(st, (str, bytes)) else list(st) for st in structures]
        motifs = [m.encode() if isinstance(m, str) else bytes(m) for st in lists for m in st]
        data = np.frombuffer(b"".join(motifs) + b"\0", np.uint8).copy()
        motif_off = np.concatenate([[0], np.cumsum([len(m) for m in motifs], dtype=np.int64)]).astype(np.int64)
        struct_off = np.concatenate([[0], np.cumsum([len(st) for st in lists], dtype=np.int64)]).astype(np.int32)
        if not isinstance(off, torch.Tensor) or off.dim() != 1 or off.numel() < 1 or not isinstance(bases, torch.Tensor) or bases.dim() != 1:
            raise MtrError("off must be a 1-D torch tensor of N + 1 offsets and bases a 1-D torch tensor")
        N, T = int(off.numel()) - 1, int(bases.numel())
        col = self._gpu_column
        ptrs = [col(off, torch.int64, (N + 1,), "the windows' off"), col(bases, torch.uint8, (T,), "the windows' bases"), col(which, torch.int32, (N,), "the windows' structure")]
        dev = torch.device("cuda", self.device)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        keep = (data, motif_off, struct_off)
        return keep, (data.ctypes.data, motif_off.ctypes.data, struct_off.ctypes.data, len(lists), *ptrs, N, T, int(gain), int(mismatch), int(indel), stream), N, dev

    def window_structure(self, structures, off, bases, which, gain: int = 1, mismatch: int = 1, indel: int = 1) -> WindowStructure:
        """The motif structure of windows (mtr_window_structure_device): window w = bases[off[w]:off[w + 1]] (codes 0..3) aligned globally to
        structures[which[w]], an ordered list of motifs each repeated zero or more whole times; per segment its span, copies and matches.
        structures: a sequence of structures, each a string (one motif) or a sequence of strings - at most 2 motifs of 32 bases in all, or 4 of
        16.  off (int64 [N + 1]), bases (uint8 [T]) and which (int32 [N]) are tensors on this engine's device: genotype_windows' off and bases
        with which = sg.locus, or allele_consensus' off and bases with which = arange(2 * n_loci) // 2.  A window above WS_MAX_WINDOW bases is
        marked skipped.  Needs no upload and no run and changes nothing either left.  Returns a WindowStructure of fresh tensors on this
        engine's device; stream handling as call_alleles'."""
        import torch

        keep, args, N, dev = self._window_args(structures, off, bases, which, gain, mismatch, indel)
        ws = WindowStructure(torch.empty((N, 4, 4), dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                             torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.uint8, device=dev))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CWindowStructureDst(*[t.data_ptr() if t.numel() else None for t in ws], N)
        self._check(self.lib.mtr_window_structure_device(self.h, *args, C.byref(dst)), "mtr_window_structure_device")
        del keep
        return ws

    def window_edits(self, structures, off, bases, which, gain: int = 1, mismatch: int = 1, indel: int = 1) -> WindowEdits:
        """The edits of windows (mtr_window_edits_device, mtr_window_edits_copy_device): the alignment path of Engine.window_structure for the
        same arguments, read out - every substitution, insertion and deletion with its window position, segment, copy of the segment's motif,
        column of the motif and base, in path order, window w's at edits[off[w]:off[w + 1]].  seg, score and skipped are window_structure's.
        The arguments and their limits are window_structure's.  Needs no upload and no run and changes nothing either left.  Returns a
        WindowEdits of fresh tensors on this engine's device; stream handling as window_structure's."""
        import torch

        keep, args, N, dev = self._window_args(structures, off, bases, which, gain, mismatch, indel)
        n_edits = C.c_int64(0)
        self._check(self.lib.mtr_window_edits_device(self.h, *args, C.byref(n_edits)), "mtr_window_edits_device")
        del keep
        E = int(n_edits.value)
        we = WindowEdits(torch.empty(N + 1, dtype=torch.int64, device=dev), torch.empty((E, WE_FIELDS), dtype=torch.int32, device=dev),
                         torch.empty((N, 4, 4), dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.uint8, device=dev))
        torch.cuda.current_stream(dev).synchronize()            # the library writes the columns on its own stream: torch's earlier use of the memory is done
        dst = CWindowEditsDst(*[t.data_ptr() if t.numel() else None for t in we], N, E)
        self._check(self.lib.mtr_window_edits_copy_device(self.h, C.byref(dst)), "mtr_window_edits_copy_device")
        return we

    def test_window_edits_rounds(self) -> int:
        """mtr_test_window_edits_rounds: the rounds the last window_edits call took (MTR_TEST_WE_SCRATCH_BYTES caps a round's transient bytes)"""
        rounds = C.c_int32(0)
        self._check(self.lib.mtr_test_window_edits_rounds(self.h, C.byref(rounds)), "mtr_test_window_edits_rounds")
        return int(rounds.value)

    def test_catalog_stats(self):
        """mtr_test_catalog_stats: what the last genotype_catalog call saw - (positions, passed by the filter, seed hits, candidates) and the
        host-clock ms of (index build and upload, first scan pass, the rest)"""
        counts, ms = (C.c_int64 * 4)(), (C.c_double * 3)()
        self._check(self.lib.mtr_test_catalog_stats(self.h, counts, ms), "mtr_test_catalog_stats")
        return tuple(int(v) for v in counts), tuple(float(v) for v in ms)

    def test_partial_catalog_stats(self):
        """mtr_test_partial_catalog_stats: what the last genotype_partial_catalog call saw - (positions, passed by the filter, seed hits,
        candidates) and the host-clock ms of (index build and upload, first scan pass, the rest)"""
        counts, ms = (C.c_int64 * 4)(), (C.c_double * 3)()
        self._check(self.lib.mtr_test_partial_catalog_stats(self.h, counts, ms), "mtr_test_partial_catalog_stats")
        return tuple(int(v) for v in counts), tuple(float(v) for v in ms)

    def test_catalog_build_stats(self):
        """mtr_test_catalog_build_stats: the host-clock ms of this engine's last build_catalog - (the host's pass over the lengths, the uploads,
        the device build)"""
        ms = (C.c_double * 3)()
        self._check(self.lib.mtr_test_catalog_build_stats(self.h, ms), "mtr_test_catalog_build_stats")
        return tuple(float(v) for v in ms)

    def test_unit_motifs(self, units, read=None, copies=None, repeat_len=None, table_slots: int = 0) -> ReportMotifs:
        """mtr_test_unit_motifs: the kernels of report_motif_tensors on caller-given units, one bytes (or str) per unit.  read: the read of
        each unit, non-decreasing (default: every unit a read of its own); copies: num_freq_unit (default 1); repeat_len (default: the
        unit's length); table_slots: 0 or a power of two above len(units), the size of the grouping's table.  Returns a ReportMotifs of
        numpy arrays."""
        n = len(units)
        udata, uoff = pack_ids(units, n)

        def col(a, default):
            a = np.ascontiguousarray(default if a is None else a, np.int32)
            if a.shape != (n,):
                raise MtrError(f"{a.shape} values for {n} units")
            return a
        rd = col(read, np.arange(n))
        cp = col(copies, np.ones(n))
        ln = col(repeat_len, np.diff(uoff))
        p8, p32, p64 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        strand, rotation, motif_len, group, motif_off, motifs = p8(), p32(), p32(), p32(), p64(), p8()
        g_first, g_repeats, g_reads, g_copies, g_bases = p32(), p32(), p32(), p64(), p64()
        ng = C.c_int64()
        outs = [strand, rotation, motif_len, group, motif_off, motifs, g_first, g_repeats, g_reads, g_copies, g_bases]
        self._check(self.lib.mtr_test_unit_motifs(self.h, n, udata.ctypes.data, uoff.ctypes.data, rd.ctypes.data, cp.ctypes.data, ln.ctypes.data, int(table_slots),
                                                  C.byref(strand), C.byref(rotation), C.byref(motif_len), C.byref(group), C.byref(ng), C.byref(motif_off),
                                                  C.byref(motifs), C.byref(g_first), C.byref(g_repeats), C.byref(g_reads), C.byref(g_copies), C.byref(g_bases)),
                    "mtr_test_unit_motifs")
        try:
            G = int(ng.value)
            take = lambda p, k: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].copy()   # noqa: E731  (every array has room for one entry)
            off = take(motif_off, G + 1)
            return ReportMotifs(take(strand, n), take(rotation, n), take(motif_len, n), take(group, n), off, take(motifs, int(off[-1])),
                                take(g_first, G), take(g_repeats, G), take(g_reads, G), take(g_copies, G), take(g_bases, G))
        finally:
            for p in outs:
                _libc.free(C.cast(p, C.c_void_p))

    def test_report_lines(self, fields, read_len, units, ids) -> List[bytes]:
        """mtr_test_report_lines: the line function of report_text on caller-given rows - fields int32 [n, 14], read_len [n], units
        and ids one bytes (or str) per row.  Returns per row its line."""
        f = np.ascontiguousarray(np.asarray(fields, np.int32).reshape(-1, 14))
        ln = np.ascontiguousarray(read_len, np.int32)
        udata, uoff = pack_ids(units, len(f))
        idata, ioff = pack_ids(ids, len(f))
        if len(ln) != len(f):
            raise MtrError(f"{len(ln)} read lengths for {len(f)} rows")
        pt, po = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int64)()
        self._check(self.lib.mtr_test_report_lines(self.h, len(f), f.ctypes.data, ln.ctypes.data, udata.ctypes.data, uoff.ctypes.data,
                                                   idata.ctypes.data, ioff.ctypes.data, C.byref(pt), C.byref(po)), "mtr_test_report_lines")
        try:
            off = np.ctypeslib.as_array(po, shape=(len(f) + 1,)).copy()
            text = C.string_at(pt, int(off[-1]))
            return [text[int(off[k]):int(off[k + 1])] for k in range(len(f))]
        finally:
            _libc.free(C.cast(pt, C.c_void_p))
            _libc.free(C.cast(po, C.c_void_p))

    def test_chain(self, sets):
        """mtr_test_chain: the report's chain kernel on caller-given records; sets = list of (start, end, matches) sequences.
        Returns per set its chain (indices within the set, print order)."""
        off = np.zeros(len(sets) + 1, np.int64)
        off[1:] = np.cumsum([len(s[0]) for s in sets])
        cols = [np.ascontiguousarray(np.concatenate([np.asarray(s[c], np.int32) for s in sets]) if len(sets) else np.zeros(0, np.int32), np.int32)
                for c in range(3)]
        pl, pi = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        self._check(self.lib.mtr_test_chain(self.h, len(sets), off.ctypes.data, cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data,
                                            C.byref(pl), C.byref(pi)), "mtr_test_chain")
        try:
            return [[pi[int(off[k]) + t] for t in range(pl[k])] for k in range(len(sets))]
        finally:
            _libc.free(C.cast(pl, C.c_void_p))
            _libc.free(C.cast(pi, C.c_void_p))

    def process_in_file(self, reads: Sequence[np.ndarray], file_state: "FileState") -> List[List[Record]]:
        """the next reads of a file under the reference's whole-file behaviour (include/mtr_hip.h, file-order mode)"""
        self.upload(reads, file_state)
        self.run()
        return self.fetch()

    def run(self):
        self._check(self.lib.mtr_run_resident(self.h), "mtr_run_resident")

    def run_async(self):
        """enqueue K1 + K2 on the context's stream without waiting (mtr_run_resident_async)"""
        self._check(self.lib.mtr_run_resident_async(self.h), "mtr_run_resident_async")

    def wait(self):
        self._check(self.lib.mtr_wait(self.h), "mtr_wait")

    def last_mode(self) -> str:
        """how the last launch ran (mtr_test_last_mode)"""
        return {0: "per-read kernel", 2: "staged chain"}.get(int(self.lib.mtr_test_last_mode(self.h)), "?")

    def fetch(self) -> List[List[Record]]:
        recs = C.POINTER(CRecord)()
        cnts = C.POINTER(C.c_int32)()
        total = C.c_int64()
        self._check(self.lib.mtr_fetch_results(self.h, C.byref(recs), C.byref(cnts), C.byref(total)), "mtr_fetch_results")
        try:
            return self._unpack(recs, cnts, self.n_reads)
        finally:
            self.lib.mtr_free_results(recs, cnts)

    def process(self, reads: Sequence[np.ndarray]) -> List[List[Record]]:
        """mtr_process_batch: reads = sequences of base codes 0..3; returns per read its records in insertion order."""
        bases, offs, lens = _flatten(reads)
        recs = C.POINTER(CRecord)()
        cnts = C.POINTER(C.c_int32)()
        total = C.c_int64()
        self.n_reads = len(reads)                       # (before the call: after MTR_ERR_DP_TOO_LARGE the reads before the failing one are still fetched)
        self._check(self.lib.mtr_process_batch(self.h, bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(reads),
                                               C.byref(recs), C.byref(cnts), C.byref(total)), "mtr_process_batch")
        try:
            return self._unpack(recs, cnts, len(reads))
        finally:
            self.lib.mtr_free_results(recs, cnts)

    @staticmethod
    def _unpack(recs, cnts, n) -> List[List[Record]]:
        out, p = [], 0
        for i in range(n):
            lst = []
            for _ in range(cnts[i]):
                r = recs[p]
                p += 1
                per = r.rep_period
                lst.append(Record(r.rep_start, r.rep_end, r.repeat_len, per, r.num_freq_unit, r.num_matches, r.num_mismatches,
                                  r.num_insertions, r.num_deletions, r.kmer, r.match_gain, r.mismatch_penalty, r.indel_penalty,
                                  r.unit.decode(), tuple(r.unit_score[:max(0, min(per, MAX_PERIOD))])))
            out.append(lst)
        return out

    def upload_packed(self, reads: Sequence[np.ndarray]):
        """the host's own packing (mtr_upload_batch_packed): reads -> the 2-bit device image, packed here with numpy"""
        lens = np.array([len(r) for r in reads], dtype=np.int32)
        nw = lens.astype(np.int64) // 16 + 4
        woff = np.zeros(len(reads), np.int64)
        if len(reads) > 1:
            woff[1:] = np.cumsum(nw[:-1])
        packed = np.zeros(int(nw.sum()), np.uint32)
        for i, r in enumerate(reads):
            packed[woff[i]: woff[i] + nw[i]] = pack_read(np.asarray(r, np.uint8))
        self._keep = (packed, woff, lens)
        self._check(self.lib.mtr_upload_batch_packed(self.h, packed.ctypes.data, len(packed), woff.ctypes.data, lens.ctypes.data, len(reads)),
                    "mtr_upload_batch_packed")
        self.n_reads = len(reads)

    def fetch_packed(self, limit: int = -1):
        """mtr_fetch_results_packed: (wire blob bytes, counts int32[n]); the blob is copied out of the context's pinned staging"""
        blob, cnts = C.c_void_p(), C.c_void_p()
        nbytes, total = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_fetch_results_packed(self.h, limit, C.byref(blob), C.byref(nbytes), C.byref(cnts), C.byref(total)), "mtr_fetch_results_packed")
        n = self.n_reads if limit < 0 else min(limit, self.n_reads)
        counts = np.ctypeslib.as_array(C.cast(cnts, C.POINTER(C.c_int32)), shape=(max(n, 1),))[:n].copy() if n > 0 and cnts.value else np.zeros(0, np.int32)
        data = C.string_at(blob, nbytes.value) if nbytes.value else b""
        return data, counts

    def fetch_packed_nocopy(self):
        """mtr_fetch_results_packed, leaving the wire form where the boundary hands it over (the context's pinned host
        buffer): returns (bytes, records)"""
        blob, cnts = C.c_void_p(), C.c_void_p()
        nbytes, total = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_fetch_results_packed(self.h, -1, C.byref(blob), C.byref(nbytes), C.byref(cnts), C.byref(total)), "mtr_fetch_results_packed")
        return int(nbytes.value), int(total.value)

    def fetch_via_wire(self) -> List[List[Record]]:
        """the records of the last run through the wire form and mtr_unpack_records (must equal fetch())"""
        data, counts = self.fetch_packed()
        total = int(counts.sum())
        recs = (CRecord * max(total, 1))()
        buf = C.create_string_buffer(data, len(data)) if data else C.create_string_buffer(1)
        st = self.lib.mtr_unpack_records(buf, len(data), total, recs)
        if st != 0:
            raise MtrError(f"mtr_unpack_records: {STATUS.get(st, st)}")
        return self._unpack(recs, counts, len(counts))

    def export_packed_device(self, device_ptr: int, capacity_bytes: int):
        """wire-form records into caller-owned device memory (for RCCL); returns (counts int32[n_reads], records, bytes)"""
        counts = np.zeros(self.n_reads, np.int32)
        total, nbytes = C.c_int64(), C.c_int64()
        self._check(self.lib.mtr_export_packed_device(self.h, C.c_void_p(device_ptr), capacity_bytes, counts.ctypes.data, C.byref(total), C.byref(nbytes)),
                    "mtr_export_packed_device")
        return counts, int(total.value), int(nbytes.value)

    def first_failed_read(self) -> int:
        v = C.c_int32()
        self.lib.mtr_get_first_failed_read(self.h, C.byref(v))
        return int(v.value)

    # ---- measurements ------------------------------------------------------------------------------------
    def kernel_times_ms(self):
        kt = (CKernelTime * 10)()
        self._check(self.lib.mtr_get_kernel_times(self.h, kt, 10), "mtr_get_kernel_times")
        out = {"k1_ranges": float(kt[0].ms), "k2_units": float(kt[1].ms)}
        for i, name in enumerate(("ranges", "unit_search", "alignments", "selection", "revisions", "finish_replay")):
            if kt[2 + i].launches:
                out["chain_" + name] = float(kt[2 + i].ms)
        # the two dominant kernels by themselves (HIP events around each launch on the launch stream; both passes of the chain summed)
        for i, name in enumerate(("mtr_k_revise_quads", "mtr_k_dp2_quads")):
            if kt[8 + i].launches:
                out["kernel_" + name] = float(kt[8 + i].ms)
        return out

    def counters(self):
        c = (C.c_int64 * len(COUNTER_NAMES))()
        self._check(self.lib.mtr_get_counters(self.h, c, len(COUNTER_NAMES)), "mtr_get_counters")
        return {n: int(c[i]) for i, n in enumerate(COUNTER_NAMES)}

    # ---- building blocks (parity tests) ----------------------------------------------------------------------
    def test_ranges(self, finder: str = "wave"):
        """The range finder alone on the uploaded batch -> per read list of (start, end, w, di_bits).  finder="wave": one wavefront per
        read (mtr_test_ranges); finder="parts": the three kernels the staged chain launches for a batch of at most 256 reads
        (mtr_test_ranges_parts; a batch the chain would not run them on: MtrError)."""
        if finder not in ("wave", "parts"):
            raise ValueError("finder is 'wave' or 'parts'")
        name = "mtr_test_ranges" if finder == "wave" else "mtr_test_ranges_parts"
        P = C.POINTER
        pc, ps, pe, pw, pd, tot = P(C.c_int32)(), P(C.c_int32)(), P(C.c_int32)(), P(C.c_int32)(), P(C.c_uint64)(), C.c_int64()
        self._check(getattr(self.lib, name)(self.h, C.byref(pc), C.byref(ps), C.byref(pe), C.byref(pw), C.byref(pd), C.byref(tot)), name)
        try:
            n, m = self.n_reads, int(tot.value)
            counts = np.ctypeslib.as_array(pc, shape=(n,)).tolist()
            cols = [np.ctypeslib.as_array(q, shape=(m,)).tolist() if m else [] for q in (ps, pe, pw, pd)]
        finally:
            for ptr in (pc, ps, pe, pw, pd):
                _libc.free(C.cast(ptr, C.c_void_p))
        rows = list(zip(*cols))
        out, p = [], 0
        for c in counts:
            out.append(rows[p:p + c])
            p += c
        return out

    def test_file_tail(self):
        """mtr_test_file_tail: what file-order mode gave the resident batch - (tail uint16, tail_off int64 [n + 1], after uint8 [n, 2]):
        read i's stale entries of inputString_w_rand are tail[tail_off[i]:tail_off[i + 1]], after[i] its orgInputString[L], [L + 1].
        Empty tails and zeros after an isolated upload."""
        P = C.POINTER
        tl, to, af = P(C.c_uint16)(), P(C.c_int64)(), P(C.c_uint8)()
        self._check(self.lib.mtr_test_file_tail(self.h, C.byref(tl), C.byref(to), C.byref(af)), "mtr_test_file_tail")
        n = self.n_reads
        try:
            tail_off = np.ctypeslib.as_array(to, shape=(n + 1,)).copy()
            m = int(tail_off[n])
            tail = np.ctypeslib.as_array(tl, shape=(m,)).copy() if m else np.zeros(0, np.uint16)
            after = np.ctypeslib.as_array(af, shape=(n, 2)).copy()
        finally:
            for a in (tl, to, af):
                _libc.free(C.cast(a, C.c_void_p))
        return tail, tail_off, after

    @staticmethod
    def _dp_task_arrays(tasks, pad_units: bool):
        """The seven arrays of mtr_test_wrap_dp's tasks (read_idx, qs, qe, unit codes, G, MM, D), in the order the two DP entry points take them.
        pad_units: one byte behind the units, so that no task at all is still an array."""
        rd = np.array([t[0] for t in tasks], np.int32)
        qs = np.array([t[1] for t in tasks], np.int32)
        qe = np.array([t[2] for t in tasks], np.int32)
        uo = np.zeros(len(tasks) + 1, np.int32)
        uo[1:] = np.cumsum([len(t[3]) for t in tasks])
        units = np.ascontiguousarray(np.concatenate([np.asarray(t[3], np.uint8) for t in tasks] + ([np.zeros(1, np.uint8)] if pad_units else [])))
        g = np.array([t[4] for t in tasks], np.int32)
        m = np.array([t[5] for t in tasks], np.int32)
        d = np.array([t[6] for t in tasks], np.int32)
        return rd, qs, qe, units, uo, g, m, d

    def test_wrap_dp(self, tasks):
        """tasks: list of (read_idx, qs, qe, unit codes, G, MM, D) -> int32 [n,8] as wrap_around_DP_sub returns."""
        n = len(tasks)
        arrays = self._dp_task_arrays(tasks, pad_units=False)
        out = np.zeros((n, 8), np.int32)
        self._check(self.lib.mtr_test_wrap_dp(self.h, n, *(a.ctypes.data for a in arrays), out.ctypes.data), "mtr_test_wrap_dp")
        return out

    def test_polish(self, tasks):
        """mtr_test_polish: polish_repeat on one wavefront per task.  tasks: list of (read_idx, rep_start, rep_end, k, unit codes, node frequencies)
        -> list of polished units (uint8 codes)."""
        n = len(tasks)
        rd, rs, re, kk = (np.array([t[i] for t in tasks], np.int32) for i in range(4))
        uo = np.zeros(n + 1, np.int32)
        uo[1:] = np.cumsum([len(t[4]) for t in tasks])
        units = np.ascontiguousarray(np.concatenate([np.asarray(t[4], np.uint8) for t in tasks]))
        scores = np.ascontiguousarray(np.concatenate([np.asarray(t[5], np.int32) for t in tasks]))
        out_units, out_len = np.zeros((n, 500), np.uint8), np.zeros(n, np.int32)
        self._check(self.lib.mtr_test_polish(self.h, n, rd.ctypes.data, rs.ctypes.data, re.ctypes.data, kk.ctypes.data, units.ctypes.data,
                                             scores.ctypes.data, uo.ctypes.data, out_units.ctypes.data, out_len.ctypes.data), "mtr_test_polish")
        return [out_units[i, :out_len[i]].copy() for i in range(n)]

    REVISE_MODES = {"WAVE": 0, "SLOTS": 1}                  # MTR_TEST_REVISE_* of include/mtr_hip_test.h

    def test_revise(self, mode: str, groups, waves: int = 0):
        """mtr_test_revise: revise_representative_unit on chosen records and units of the uploaded batch.  groups: list of groups, a group a list of tasks
        (read_idx, rr, unit codes, node frequencies), rr = the record's 13 scalar fields (rep_start, rep_end, repeat_len, period, copies, mat, mis, ins, del,
        k, G, MM, D).  mode "WAVE": revise() - polish first - on one wavefront per group, the round memo living across the group's tasks; "SLOTS":
        mtr_k_revise_quads itself on `waves` wavefronts (0: one) over the tasks in the order given, the units being polished ones.
        -> (list of (rr 13-tuple, unit uint8 codes) per task in the order given, the launch's cell budget per wavefront).  Engine.counters() describes the launch."""
        tasks = [t for g in groups for t in g]
        n = len(tasks)
        go = np.zeros(len(groups) + 1, np.int32)
        go[1:] = np.cumsum([len(g) for g in groups])
        rd = np.array([t[0] for t in tasks] + [0], np.int32)
        rr = np.ascontiguousarray(np.array([list(t[1]) for t in tasks] + [[0] * 13], np.int32).reshape(-1, 13))
        uo = np.zeros(n + 1, np.int32)
        uo[1:] = np.cumsum([len(t[2]) for t in tasks])
        units = np.ascontiguousarray(np.concatenate([np.asarray(t[2], np.uint8) for t in tasks] + [np.zeros(1, np.uint8)]))
        scores = np.ascontiguousarray(np.concatenate([np.asarray(t[3], np.int32) for t in tasks] + [np.zeros(1, np.int32)]))
        if any(len(t[2]) != len(t[3]) for t in tasks):
            raise ValueError("a task's node frequencies are one per unit base")
        out_rr, out_units, cells = np.zeros((max(n, 1), 13), np.int32), np.zeros((max(n, 1), 500), np.uint8), C.c_int64(0)
        self._check(self.lib.mtr_test_revise(self.h, self.REVISE_MODES[mode], len(groups), go.ctypes.data, rd.ctypes.data, rr.ctypes.data, units.ctypes.data,
                                             scores.ctypes.data, uo.ctypes.data, int(waves), out_rr.ctypes.data, out_units.ctypes.data, C.byref(cells)),
                    "mtr_test_revise")
        return [(tuple(int(v) for v in out_rr[i]), out_units[i, :max(0, min(int(out_rr[i, 3]), 500))].copy()) for i in range(n)], int(cells.value)

    DP_PASSES = {"WAVE2P": 0, "Q4": 1, "QUAD2P": 2, "FOUR1P": 3, "OCT1P": 4, "OCT2P": 5}       # MTR_TEST_PASS_* of include/mtr_hip_test.h

    def test_wrap_dp_pass(self, dp_pass: str, groups):
        """mtr_test_wrap_dp_pass: one chosen forward pass of the wrap-around DP with its tracebacks.  groups: list of groups, a group a list of
        test_wrap_dp's tasks (the DPs that share one forward pass) -> int32 [n tasks, 2, 8]: per task (in the order given) and parameter set what
        wrap_around_DP_sub returns.  The two-parameter passes: set 0 = (1,1,3), set 1 = (1,3,1); the one-parameter passes fill set 0 with the task's own."""
        tasks = [t for g in groups for t in g]
        n = len(tasks)
        go = np.zeros(len(groups) + 1, np.int32)
        go[1:] = np.cumsum([len(g) for g in groups])
        arrays = self._dp_task_arrays(tasks, pad_units=True)
        out = np.zeros((max(n, 1), 2, 8), np.int32)
        self._check(self.lib.mtr_test_wrap_dp_pass(self.h, self.DP_PASSES[dp_pass], len(groups), go.ctypes.data, *(a.ctypes.data for a in arrays), out.ctypes.data),
                    "mtr_test_wrap_dp_pass")
        return out[:n]

    def set_trace(self, max_events: int):
        self._check(self.lib.mtr_set_trace(self.h, max_events), "mtr_set_trace")

    def get_trace(self) -> np.ndarray:
        ev = C.POINTER(C.c_int32)()
        n = C.c_int64()
        self._check(self.lib.mtr_get_trace(self.h, C.byref(ev), C.byref(n)), "mtr_get_trace")
        arr = np.ctypeslib.as_array(ev, shape=(max(n.value, 1), 16))[: n.value].copy()
        _libc.free(C.cast(ev, C.c_void_p))
        return arr


def _c_float_text(x) -> str:
    """printf("%f", (double)x) as glibc prints it: Python's "%f" is the same correctly rounded conversion, except for the
    spelling of infinities and NaNs (glibc keeps the sign of a NaN: an x86 host's 0.0f / 0 prints "-nan")"""
    x = float(x)
    if x != x:
        return "-nan" if np.signbit(x) else "nan"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return "%f" % x


def format_report(ids, lens, report: Report, alignments: "ReportAlignments | None" = None) -> bytes:
    """mTR's report lines (mtr_amd/host/print.c: report_line) from a Report: per repeat ID, L, start+1, end+1, repeat_len, period,
    copies, matches, ratio (%f of the float), mismatches, insertions, deletions, unit, tab-separated.
    ids: per read its ID (str or bytes, what the FASTA header line holds after '>'), lens: per read its length.
    alignments (Engine.report_alignment_tensors of the same run): mTR -a's output - after each repeat's line the block print.c's
    alignment_block prints: an empty line, the scores line, an empty line, then per ALIGN_WIDTH columns the three rows and an empty line."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    read, fields, ratio = host(report.read), host(report.fields).reshape(-1, 14), host(report.ratio).astype(np.float32)
    unit_off, units = host(report.unit_off), host(report.units).tobytes()
    if alignments is not None:
        col_off, text = host(alignments.col_off), np.ascontiguousarray(host(alignments.text), np.uint8)
        text = text.reshape(3, text.size // 3)
        rows = [text[0].tobytes(), text[1].tobytes(), text[2].tobytes()]
        if len(col_off) != len(read) + 1:
            raise MtrError(f"alignments of {len(col_off) - 1} repeats for a report of {len(read)}")
    out = []
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    for k in range(len(read)):
        r = int(read[k])
        f = [int(v) for v in fields[k]]
        cols = [str(int(lens[r])), str(f[0] + 1), str(f[1] + 1), str(f[2]), str(f[3]), str(f[4]), str(f[5]), _c_float_text(ratio[k]),
                str(f[6]), str(f[7]), str(f[8])]
        out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + units[int(unit_off[k]):int(unit_off[k + 1])] + b"\n")
        if alignments is not None:
            out.append(f"\nmatch gain = {f[10]}, mismatch penalty = {f[11]}, indel penalty = {f[12]}\n\n".encode())
            c1 = int(col_off[k + 1])
            for c in range(int(col_off[k]), c1, ALIGN_WIDTH):
                e = min(c + ALIGN_WIDTH, c1)
                out.append(rows[0][c:e] + b"\n" + rows[1][c:e] + b"\n" + rows[2][c:e] + b"\n\n")
    return b"".join(out)


_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def canonical_motif(unit):
    """(motif, strand, rotation) of one unit (str or bytes over ACGT) as include/mtr_hip.h defines them: the least string among the
    rotations of the unit and of its reverse complement, cut to its primitive period; strand 0 if a rotation of the unit itself is
    that string, rotation the smallest one on that strand.  Pure Python; the motif comes back in the type the unit came in."""
    u = unit.encode() if isinstance(unit, str) else bytes(unit)
    p = len(u)
    if p == 0:
        return unit[:0], 0, 0
    best = None
    for strand, s in enumerate((u, u.translate(_COMPLEMENT)[::-1])):
        d = s + s
        r = min(range(p), key=lambda r: (d[r:r + p], r))
        cand = (d[r:r + p], strand, r)
        if best is None or cand[0] < best[0]:
            best = cand
    canon, strand, rotation = best
    d = next(d for d in range(1, p + 1) if p % d == 0 and canon[d:] + canon[:d] == canon)
    motif = canon[:d]
    return (motif.decode() if isinstance(unit, str) else motif), strand, rotation


def format_motif_hits(ids, lens, motifs, hits: MotifHits, min_ratio: float = 0.0, min_copies: int = 1) -> bytes:
    """The hits of Engine.search_motifs as text, one line per kept hit in the thirteen columns of mTR's report line (format_report), so that
    what parses the report parses this: ID, L, start+1, end+1, repeat_len, U, copies, matches, ratio (%f of the float), mismatches,
    insertions, deletions, and the motif as aligned - its reverse complement for strand 1.  Reads in input order, motifs in the given order
    within a read.  Kept: score > 0 (always), ratio >= min_ratio and copies >= min_copies.
    ids, lens: per read its ID (str or bytes) and length; motifs: what search_motifs was given; hits: its result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v.encode() if isinstance(v, str) else bytes(v) for v in motifs]
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    n, m = len(bid), len(bmot)
    fields, score = host(hits.fields).reshape(n, m, 8), host(hits.score).reshape(n, m)
    ratio, strand = host(hits.ratio).astype(np.float32).reshape(n, m), host(hits.strand).reshape(n, m)
    if len(lens) != n:
        raise MtrError(f"{len(lens)} lengths for {n} ids")
    shown = [(b, b.translate(_COMPLEMENT)[::-1]) for b in bmot]
    out = []
    for r, k in zip(*np.nonzero((score > 0) & (ratio >= np.float32(min_ratio)) & (fields[:, :, 3] >= min_copies))):
        f = [int(v) for v in fields[r, k]]
        cols = [str(int(lens[r])), str(f[0] + 1), str(f[1] + 1), str(f[2]), str(len(bmot[k])), str(f[3]), str(f[4]), _c_float_text(ratio[r, k]),
                str(f[5]), str(f[6]), str(f[7])]
        out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + shown[k][int(strand[r, k])] + b"\n")
    return b"".join(out)


def format_motif_loci(ids, lens, motifs, loci: MotifLoci, min_ratio: float = 0.0, min_copies: int = 1) -> bytes:
    """The loci of Engine.search_motif_loci as text: format_motif_hits' thirteen columns, one line per kept locus, ordered by read, then motif
    (in the given order), then start.  Strand 1 prints the motif's reverse complement.  Kept: ratio >= min_ratio and copies >= min_copies.
    ids, lens: per read its ID (str or bytes) and length; motifs: what search_motif_loci was given; loci: its result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v.encode() if isinstance(v, str) else bytes(v) for v in motifs]
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    n, m = len(bid), len(bmot)
    off, fields = host(loci.loci_off).reshape(-1), host(loci.fields).reshape(-1, 8)
    score, ratio, strand = host(loci.score).reshape(-1), host(loci.ratio).astype(np.float32).reshape(-1), host(loci.strand).reshape(-1)
    if len(lens) != n:
        raise MtrError(f"{len(lens)} lengths for {n} ids")
    if len(off) != n * m + 1:
        raise MtrError(f"{len(off)} offsets for {n} ids and {m} motifs: {n * m + 1} needed")
    T = int(off[-1]) if len(off) else 0
    if not (len(fields) == len(score) == len(ratio) == len(strand) == T):
        raise MtrError(f"columns of {len(fields)}, {len(score)}, {len(ratio)} and {len(strand)} rows for {T} loci")
    if int(off[0]) != 0 or (np.diff(off) < 0).any():
        raise MtrError("loci_off does not ascend from 0")
    shown = [(b, b.translate(_COMPLEMENT)[::-1]) for b in bmot]
    out = []
    for p in range(n * m):
        r, k = divmod(p, m)
        for t in range(int(off[p]), int(off[p + 1])):
            f = [int(v) for v in fields[t]]
            if not (ratio[t] >= np.float32(min_ratio) and f[3] >= min_copies):
                continue
            cols = [str(int(lens[r])), str(f[0] + 1), str(f[1] + 1), str(f[2]), str(len(bmot[k])), str(f[3]), str(f[4]), _c_float_text(ratio[t]),
                    str(f[5]), str(f[6]), str(f[7])]
            out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + shown[k][int(strand[t])] + b"\n")
    return b"".join(out)


def format_flank_hits(ids, lens, patterns, hits: FlankHits, max_dist: "int | None" = None) -> bytes:
    """The hits of Engine.search_flanks as text, one tab-separated line per kept hit: ID, L, pattern index, strand, dist, start + 1 (1-origin),
    end (1-origin, inclusive; an empty match prints start + 1 and end one below it), the pattern's length, and the pattern as matched - its
    reverse complement for strand 1.  Reads in input order, patterns in the given order within a read.  Kept: dist <= max_dist (None: all).
    ids, lens: per read its ID (str or bytes) and length; patterns: what search_flanks was given; hits: its result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bpat = [v.encode() if isinstance(v, str) else bytes(v) for v in patterns]
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    n, m = len(bid), len(bpat)
    dist, start, end, strand = (host(t).reshape(n, m) for t in hits)
    if len(lens) != n:
        raise MtrError(f"{len(lens)} lengths for {n} ids")
    shown = [(b, b.translate(_COMPLEMENT)[::-1]) for b in bpat]
    out = []
    for r in range(n):
        for k in range(m):
            if max_dist is not None and int(dist[r, k]) > max_dist:
                continue
            cols = [str(int(lens[r])), str(k), str(int(strand[r, k])), str(int(dist[r, k])), str(int(start[r, k]) + 1), str(int(end[r, k])), str(len(bpat[k]))]
            out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + shown[k][int(strand[r, k])] + b"\n")
    return b"".join(out)


def format_genotypes(ids, lens, loci, gt: Genotypes) -> bytes:
    """The rows of Engine.genotype_loci as text, one tab-separated line per SPANNING (read, locus): ID, L, locus index, orientation, the left
    and the right flank's distance, the window's start (1-origin) and end (inclusive), the allele's length in bases, copies, matches, ratio (%f
    of the float), mismatches, insertions, deletions, and the motif as aligned - its reverse complement for orientation 1.  Reads in input
    order, loci in the given order within a read.
    ids, lens: per read its ID (str or bytes) and length; loci: what genotype_loci was given; gt: its result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v[1].encode() if isinstance(v[1], str) else bytes(v[1]) for v in loci]
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    n, m = len(bid), len(bmot)
    spanning, orientation = host(gt.spanning).reshape(n, m), host(gt.orientation).reshape(n, m)
    fdist, window, fields = host(gt.flank_dist).reshape(n, m, 2), host(gt.window).reshape(n, m, 2), host(gt.fields).reshape(n, m, 8)
    ratio = host(gt.ratio).astype(np.float32).reshape(n, m)
    if len(lens) != n:
        raise MtrError(f"{len(lens)} lengths for {n} ids")
    shown = [(b, b.translate(_COMPLEMENT)[::-1]) for b in bmot]
    out = []
    for r, k in zip(*np.nonzero(spanning)):
        f = [int(v) for v in fields[r, k]]
        lo, hi = int(window[r, k, 0]), int(window[r, k, 1])
        cols = [str(int(lens[r])), str(k), str(int(orientation[r, k])), str(int(fdist[r, k, 0])), str(int(fdist[r, k, 1])), str(lo + 1), str(hi), str(hi - lo),
                str(f[3]), str(f[4]), _c_float_text(ratio[r, k]), str(f[5]), str(f[6]), str(f[7])]
        out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + shown[k][int(orientation[r, k])] + b"\n")
    return b"".join(out)


def catalog_loci_args(loci, max_flank_dist: int, seed_len: "int | None"):
    """What Engine.genotype_catalog and Engine.genotype_partial_catalog make of their loci: the checks of the list's shape, the sequences packed
    as the C calls take them (seqs, seq_off), the number of loci, and the seed length - pick_seed_len's where none is given"""
    if isinstance(loci, (str, bytes, bytearray)) or not hasattr(loci, "__len__"):
        raise MtrError(f"loci must be a sequence of (left_flank, motif, right_flank), got {type(loci).__name__}")
    flat = []
    for k, locus in enumerate(loci):
        if isinstance(locus, (str, bytes, bytearray)) or not hasattr(locus, "__len__") or len(locus) != 3:
            raise MtrError(f"locus {k} must be (left_flank, motif, right_flank)")
        flat.extend(locus)
    if seed_len is None:
        seed_len = pick_seed_len(loci, max_flank_dist)
    data, off = pack_ids(flat)
    return data, off, len(loci), seed_len


def pick_seed_len(loci, max_flank_dist: int) -> int:
    """The seed length Engine.genotype_catalog takes by default: the largest q <= 16 with (max_flank_dist + 1) * q bases in every flank of loci
    (a sequence of (left_flank, motif, right_flank)); raises MtrError where that is below 8 - the flanks are too short for an exact screen at
    this distance."""
    if isinstance(max_flank_dist, bool) or not isinstance(max_flank_dist, (int, np.integer)) or max_flank_dist < 0:
        raise MtrError(f"max_flank_dist must be an integer >= 0, got {max_flank_dist!r}")
    if len(loci) == 0:
        raise MtrError("loci is empty: at least one locus is needed")
    shortest, where = min((len(locus[2 * side]), (k, side)) for k, locus in enumerate(loci) for side in (0, 1))
    q = min(16, shortest // (int(max_flank_dist) + 1))
    if q < 8:
        raise MtrError(f"locus {where[0]}, {'right' if where[1] else 'left'} flank: {shortest} bases admit seeds of {q} bases at max_flank_dist = {max_flank_dist}, "
                       "fewer than 8")
    return q


def format_sparse_genotypes(ids, lens, loci, sg: SparseGenotypes) -> bytes:
    """The rows of Engine.genotype_catalog as text: byte for byte format_genotypes of the dense result, without building it.
    ids, lens: per read its ID (str or bytes) and length; loci: what genotype_catalog was given; sg: its result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v[1].encode() if isinstance(v[1], str) else bytes(v[1]) for v in loci]
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    if len(lens) != len(bid):
        raise MtrError(f"{len(lens)} lengths for {len(bid)} ids")
    if (len(bid), len(bmot)) != (sg.n_reads, sg.n_loci):
        raise MtrError(f"{len(bid)} ids and {len(bmot)} loci for the rows of {sg.n_reads} reads and {sg.n_loci} loci")
    read, locus, orientation = host(sg.read), host(sg.locus), host(sg.orientation)
    fdist, window, fields, ratio = host(sg.flank_dist), host(sg.window), host(sg.fields), host(sg.ratio).astype(np.float32)
    shown = [(b, b.translate(_COMPLEMENT)[::-1]) for b in bmot]
    out = []
    for i in range(len(read)):
        r, k, f = int(read[i]), int(locus[i]), [int(v) for v in fields[i]]
        lo, hi = int(window[i, 0]), int(window[i, 1])
        cols = [str(int(lens[r])), str(k), str(int(orientation[i])), str(int(fdist[i, 0])), str(int(fdist[i, 1])), str(lo + 1), str(hi), str(hi - lo),
                str(f[3]), str(f[4]), _c_float_text(ratio[i]), str(f[5]), str(f[6]), str(f[7])]
        out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + shown[k][int(orientation[i])] + b"\n")
    return b"".join(out)


def format_partial_genotypes(ids, lens, loci, pg: PartialGenotypes) -> bytes:
    """The rows of Engine.genotype_partial as text, one tab-separated line per PARTIAL (read, locus): ID, L, locus index, slot, the flank's
    distance, the repeat's start (1-origin) and end (inclusive) - the end is start - 1 where nothing extends -, its length in bases, copies -
    with ">=" in front where the row is open -, matches, ratio (%f of the float), score, tail, and the motif as aligned - its reverse complement
    for slots 2 and 3.  Reads in input order, loci in the given order within a read.
    ids, lens: per read its ID (str or bytes) and length; loci: what genotype_partial was given; pg: its result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v[1].encode() if isinstance(v[1], str) else bytes(v[1]) for v in loci]
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    n, m = len(bid), len(bmot)
    partial, slot, fdist = host(pg.partial).reshape(n, m), host(pg.slot).reshape(n, m), host(pg.flank_dist).reshape(n, m)
    window, ext, is_open = host(pg.window).reshape(n, m, 2), host(pg.ext).reshape(n, m, 6), host(pg.open).reshape(n, m)
    ratio = host(pg.ratio).astype(np.float32).reshape(n, m)
    if len(lens) != n:
        raise MtrError(f"{len(lens)} lengths for {n} ids")
    shown = [(b, b.translate(_COMPLEMENT)[::-1]) for b in bmot]
    out = []
    for r, k in zip(*np.nonzero(partial)):
        e = [int(v) for v in ext[r, k]]
        s, lo, hi = int(slot[r, k]), int(window[r, k, 0]), int(window[r, k, 1])
        start, end = (lo, lo + e[0]) if s in (0, 3) else (hi - e[0], hi)
        cols = [str(int(lens[r])), str(k), str(s), str(int(fdist[r, k])), str(start + 1), str(end), str(e[0]), (">=" if is_open[r, k] else "") + str(e[2]),
                str(e[3]), _c_float_text(ratio[r, k]), str(e[4]), str(e[5])]
        out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + shown[k][s >> 1] + b"\n")
    return b"".join(out)


def format_sparse_partial_genotypes(ids, lens, loci, spg: "SparsePartialGenotypes") -> bytes:
    """The rows of Engine.genotype_partial_catalog as text: byte for byte format_partial_genotypes of the dense result, without building it.
    ids, lens: per read its ID (str or bytes) and length; loci: what genotype_partial_catalog was given; spg: its result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v[1].encode() if isinstance(v[1], str) else bytes(v[1]) for v in loci]
    bid = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    if len(lens) != len(bid):
        raise MtrError(f"{len(lens)} lengths for {len(bid)} ids")
    if (len(bid), len(bmot)) != (spg.n_reads, spg.n_loci):
        raise MtrError(f"{len(bid)} ids and {len(bmot)} loci for the rows of {spg.n_reads} reads and {spg.n_loci} loci")
    read, locus, slot, fdist = host(spg.read), host(spg.locus), host(spg.slot), host(spg.flank_dist)
    window, ext, is_open, ratio = host(spg.window), host(spg.ext), host(spg.open), host(spg.ratio).astype(np.float32)
    shown = [(b, b.translate(_COMPLEMENT)[::-1]) for b in bmot]
    out = []
    for i in range(len(read)):
        r, k, e = int(read[i]), int(locus[i]), [int(v) for v in ext[i]]
        s, lo, hi = int(slot[i]), int(window[i, 0]), int(window[i, 1])
        start, end = (lo, lo + e[0]) if s in (0, 3) else (hi - e[0], hi)
        cols = [str(int(lens[r])), str(k), str(s), str(int(fdist[i])), str(start + 1), str(end), str(e[0]), (">=" if is_open[i] else "") + str(e[2]),
                str(e[3]), _c_float_text(ratio[i]), str(e[4]), str(e[5])]
        out.append(bid[r] + b"\t" + "\t".join(cols).encode() + b"\t" + shown[k][s >> 1] + b"\n")
    return b"".join(out)


def partial_support(pg: "PartialGenotypes | SparsePartialGenotypes", calls: "AlleleCalls | None" = None, min_ratio: float = 0.0) -> PartialSupport:
    """Per locus, what the reads that do not span it say (plain torch on the tensors' own device, no kernel): the partial rows, the open rows,
    the largest copies among the open rows with ratio >= min_ratio (float32) and, with the locus' calls given, n_beyond: how many of those rows
    hold more copies than the larger called allele calls.call[:, 1] - evidence of an allele longer than the one called.  call_alleles itself
    is unchanged: these rows are lower bounds, no values to rank.  pg may also be a SparsePartialGenotypes (genotype_partial_catalog's result, or
    several batches' joined): the same per-locus results by scatter over its locus column, nothing sized reads x loci."""
    import torch

    if isinstance(pg, SparsePartialGenotypes):
        m, dev = pg.n_loci, pg.partial.device
        at = pg.locus.long()
        partial, is_open = pg.partial != 0, pg.open != 0
        copies = pg.ext[:, 2]
        good = is_open & (pg.ratio >= torch.tensor(min_ratio, dtype=torch.float32, device=dev))
        count = lambda flag: torch.zeros(m, dtype=torch.int64, device=dev).index_add(0, at, flag.long())     # noqa: E731
        zero = torch.zeros((), dtype=copies.dtype, device=dev)
        top = torch.zeros(m, dtype=copies.dtype, device=dev).scatter_reduce(0, at, torch.where(good, copies, zero), "amax", include_self=True)
        beyond = None
        if calls is not None:
            larger = calls.call[:, 1].to(dev)
            if larger.shape[0] != m:
                raise MtrError(f"{larger.shape[0]} calls for {m} loci")
            beyond = count(good & (copies > larger[at]))
        return PartialSupport(count(partial), count(is_open), top, beyond)
    partial, is_open = pg.partial != 0, pg.open != 0
    copies = pg.ext[:, :, 2]
    good = is_open & (pg.ratio >= torch.tensor(min_ratio, dtype=torch.float32, device=pg.ratio.device))
    zero = torch.zeros((), dtype=copies.dtype, device=copies.device)
    top = torch.where(good, copies, zero).amax(dim=0) if copies.shape[0] else torch.zeros(copies.shape[1], dtype=copies.dtype, device=copies.device)
    beyond = None
    if calls is not None:
        larger = calls.call[:, 1].to(copies.device)
        if larger.shape[0] != copies.shape[1]:
            raise MtrError(f"{larger.shape[0]} calls for {copies.shape[1]} loci")
        beyond = (good & (copies > larger[None, :])).sum(dim=0)
    return PartialSupport(partial.sum(dim=0), is_open.sum(dim=0), top, beyond)


def format_allele_calls(loci, calls: AlleleCalls) -> bytes:
    """The calls of Engine.call_alleles as text, one tab-separated line per locus in the given order: locus index, S_l (its supporting reads),
    zygosity, the two alleles' values, their supports, cost1 and cost2, the smallest and the largest supporting value (0 and 0 without
    support), and the locus' motif as given.
    loci: what genotype_loci was given, (left_flank, motif, right_flank) each; calls: call_alleles' result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v[1].encode() if isinstance(v[1], str) else bytes(v[1]) for v in loci]
    m = len(bmot)
    off, value, zyg = host(calls.support_off).reshape(-1), host(calls.value).reshape(-1), host(calls.zygosity).reshape(-1)
    if len(off) != m + 1 or len(zyg) != m:
        raise MtrError(f"{len(zyg)} calls for {m} loci")
    call, sup, cost = host(calls.call).reshape(m, 2), host(calls.call_support).reshape(m, 2), host(calls.cost).reshape(m, 2)
    out = []
    for k in range(m):
        lo, hi = int(off[k]), int(off[k + 1])
        ends = (int(value[lo]), int(value[hi - 1])) if hi > lo else (0, 0)
        cols = [k, hi - lo, int(zyg[k]), int(call[k, 0]), int(call[k, 1]), int(sup[k, 0]), int(sup[k, 1]), int(cost[k, 0]), int(cost[k, 1]), *ends]
        out.append("\t".join(str(c) for c in cols).encode() + b"\t" + bmot[k] + b"\n")
    return b"".join(out)


def format_sequence_calls(loci, sc: SequenceCalls) -> bytes:
    """The calls of Engine.call_alleles_by_sequence as text: format_allele_calls' line per locus, then for each of the two alleles its medoid's
    read (-1 without one) and its members' mean distance to that medoid as the exact fraction sum/n (0/0 without members).
    loci: what genotype_loci was given; sc: call_alleles_by_sequence's result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    lines = format_allele_calls(loci, sc.calls).split(b"\n")[:-1]
    m = len(lines)
    off, allele, dtm = host(sc.calls.support_off).reshape(-1), host(sc.calls.allele).reshape(-1), host(sc.dist_to_medoid).reshape(-1)
    medoid, zyg = host(sc.medoid).reshape(-1, 2), host(sc.calls.zygosity).reshape(-1)
    if len(medoid) != m or len(dtm) != len(allele):
        raise MtrError(f"{len(medoid)} medoid pairs for {m} loci, {len(dtm)} distances for {len(allele)} entries")
    out = []
    for k in range(m):
        lo, hi = int(off[k]), int(off[k + 1])
        cols = []
        for a in (0, 1):
            mine = [int(d) for d, x in zip(dtm[lo:hi], allele[lo:hi]) if x == a] if a < int(zyg[k]) else []
            cols += [str(int(medoid[k, a])), f"{sum(mine)}/{len(mine)}"]
        out.append(lines[k] + b"\t" + "\t".join(cols).encode() + b"\n")
    return b"".join(out)


def format_genotype_quality(loci, calls: AlleleCalls, gq: GenotypeQuality) -> bytes:
    """The result of Engine.genotype_quality as text: format_allele_calls' line per locus, then the genotype (0/0, 0/1, 1/1, or ./. without a
    call), gq, the three pl joined by commas, and scored/unscored.
    loci: what genotype_loci was given; calls: the calls that were scored; gq: genotype_quality's result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    lines = format_allele_calls(loci, calls).split(b"\n")[:-1]
    m = len(lines)
    gt, q, pl = host(gq.gt).reshape(-1), host(gq.gq).reshape(-1), host(gq.pl).reshape(-1, 3)
    scored, unscored = host(gq.scored).reshape(-1), host(gq.unscored).reshape(-1)
    if not (len(gt) == len(q) == len(pl) == len(scored) == len(unscored) == m):
        raise MtrError(f"{len(gt)} genotypes for {m} loci")
    names = {0: "0/0", 1: "0/1", 2: "1/1"}
    out = []
    for k in range(m):
        cols = [names.get(int(gt[k]), "./."), str(int(q[k])), ",".join(str(int(v)) for v in pl[k]), f"{int(scored[k])}/{int(unscored[k])}"]
        out.append(lines[k] + b"\t" + "\t".join(cols).encode() + b"\n")
    return b"".join(out)


def with_reassigned_alleles(calls: AlleleCalls, gq: GenotypeQuality) -> AlleleCalls:
    """The calls with every read moved to the allele whose sequence it fits better (gq.best) - the input of a second consensus round.  It
    applies to every locus of zygosity 2 whose best column leaves both sides non-empty: the entries are stably partitioned by best, allele =
    best, call_support is recounted and call[a] is the value at position (n_a - 1) / 2 of allele a's list (the consensus' backbone rule); cost
    is unchanged.  Every other locus is unchanged.  Torch ops only, on whatever device the tensors are on; allele_consensus takes the result
    as it is."""
    import torch

    off, allele, zyg = calls.support_off, calls.allele, calls.zygosity
    S, m = int(allele.numel()), int(zyg.numel())
    if int(gq.best.numel()) != S or int(off.numel()) != m + 1:
        raise MtrError(f"{int(gq.best.numel())} best alleles for {S} entries of {m} loci")
    dev = allele.device
    n = off[1:] - off[:-1]
    locus = torch.searchsorted(off[1:].contiguous(), torch.arange(S, dtype=torch.int64, device=dev), right=True)        # the entry's locus
    n1 = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, locus, (gq.best == 1).to(torch.int64))
    moved = (zyg == 2) & (n1 > 0) & (n1 < n)
    new_allele = torch.where(moved[locus], gq.best, allele)
    order = torch.sort(locus * 2 + torch.where(moved[locus], new_allele.to(torch.int64), torch.zeros_like(locus)), stable=True).indices
    value, read, new_allele = calls.value[order], calls.read[order], new_allele[order]
    n_a = torch.stack([n - n1, n1], dim=1)
    first = torch.stack([off[:-1], off[:-1] + n - n1], dim=1)
    at = torch.where(moved[:, None], first + (n_a - 1) // 2, torch.zeros_like(first))
    call = torch.where(moved[:, None], value[at.reshape(-1)].reshape(m, 2) if S else calls.call, calls.call)
    support = torch.where(moved[:, None], n_a.to(calls.call_support.dtype), calls.call_support)
    return AlleleCalls(off, value, read, new_allele, zyg, call, support, calls.cost)


def _cat(parts):
    if hasattr(parts[0], "detach"):
        import torch

        return torch.cat(list(parts))
    return np.concatenate([np.asarray(p) for p in parts])


def join_sparse_genotypes(parts) -> SparseGenotypes:
    """Several batches' SparseGenotypes (in file order, the same loci) as one: n_reads summed, each batch's first read's index added to its `read`,
    every column concatenated, candidates summed.  The joined rows stay sorted by (read, locus).  Tensors or numpy columns."""
    parts = list(parts)
    if not parts:
        raise MtrError("nothing to join")
    m = parts[0].n_loci
    if any(p.n_loci != m for p in parts):
        raise MtrError(f"the batches' n_loci differ: {[p.n_loci for p in parts]}")
    first, reads = 0, []
    for p in parts:
        reads.append(p.read + first)
        first += int(p.n_reads)
    if first > 2 ** 31 - 1:
        raise MtrError(f"{first} reads are more than 2^31 - 1")
    return SparseGenotypes(first, m, _cat(reads), *[_cat([p[k] for p in parts]) for k in range(3, 11)], sum(int(p.candidates) for p in parts))


def join_windows(parts) -> GenotypeWindows:
    """Several batches' GenotypeWindows, in the order of join_sparse_genotypes' parts, as one: the bases concatenated, each batch's offsets shifted
    by the bases before it.  Tensors or numpy columns."""
    parts = list(parts)
    if not parts:
        raise MtrError("nothing to join")
    before, offs = 0, []
    for k, p in enumerate(parts):
        offs.append((p.off if k == len(parts) - 1 else p.off[:-1]) + before)
        before += int(p.off[-1])
    return GenotypeWindows(_cat(offs), _cat([p.bases for p in parts]))


def join_window_qualities(parts, windows: "GenotypeWindows | None" = None):
    """Several batches' genotype_window_qualities, in the order of join_windows' parts, as one: concatenated.  windows: join_windows' result for
    the same batches; given, the joined length must be its bases'.  Tensors or numpy arrays."""
    parts = list(parts)
    if not parts:
        raise MtrError("nothing to join")
    qual = _cat(parts)
    if windows is not None and (len(qual) != int(windows.off[-1]) or len(qual) != len(windows.bases)):
        raise MtrError(f"{len(qual)} qualities for windows of {int(windows.off[-1])} bases")
    return qual


def format_window_structure(structures, ws: WindowStructure, names=None) -> bytes:
    """The result of Engine.window_structure as text, one tab-separated line per window: its name (names[w], or its index), score, ratio, and
    per segment of its structure motif*copies[start,end)matches; a skipped window's line ends in "skipped".  structures: window w's structure
    at structures[w] (the call's structures[which[w]]), or one structure for every window."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    lists = [[st] if isinstance(st, (str, bytes)) else list(st) for st in structures]
    seg, score, ratio, skipped = host(ws.seg).reshape(-1, 4, 4), host(ws.score).reshape(-1), host(ws.ratio).reshape(-1), host(ws.skipped).reshape(-1)
    if len(lists) == 1:
        lists = lists * len(seg)
    if not len(seg) == len(score) == len(ratio) == len(skipped) == len(lists):
        raise MtrError(f"{len(lists)} structures for {len(seg)} windows")
    out = []
    for w in range(len(seg)):
        head = f"{names[w] if names is not None else w}\t{int(score[w])}\t{float(ratio[w]):.4f}"
        if skipped[w]:
            out.append(head + "\tskipped\n")
            continue
        cols = []
        for s, m in enumerate(lists[w]):
            start, end, copies, matches = (int(v) for v in seg[w, s])
            cols.append(f"{m.decode() if isinstance(m, bytes) else m}*{copies}[{start},{end}){matches}")
        out.append(head + "\t" + "\t".join(cols) + "\n")
    return "".join(out).encode()


def format_window_edits(structures, we: WindowEdits, names=None) -> bytes:
    """The result of Engine.window_edits as text, one tab-separated line per window: its name (names[w], or its index), the number of its edits,
    then one token per edit in path order; a skipped window's line is name, 0, "skipped".  structures: window w's structure at structures[w]
    (the call's structures[which[w]]), or one structure for every window.  The token grammar:
        token    = motif "#" copy ":" column change "@" pos
        change   = motif_base ">" window_base      a substitution: the motif's base at that column, the window's base at pos
                 | "+" window_base                 an insertion after that column: the window's base at pos has no motif base
                 | "-" motif_base                  a deletion of that column before pos: the motif's base has no window base
    motif is the segment's motif as given, copy and column count from 0, pos is the window position, bases are letters of ACGT: the CAA in
    copy 10 of a CAG tract is CAG#10:2G>A@32."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    lists = [[st] if isinstance(st, (str, bytes)) else list(st) for st in structures]
    off, edits, skipped = host(we.off).reshape(-1), host(we.edits).reshape(-1, WE_FIELDS), host(we.skipped).reshape(-1)
    if len(lists) == 1:
        lists = lists * len(skipped)
    if not len(off) - 1 == len(skipped) == len(lists):
        raise MtrError(f"{len(lists)} structures for {len(skipped)} windows")
    out = []
    for w in range(len(skipped)):
        name = names[w] if names is not None else w
        if skipped[w]:
            out.append(f"{name}\t0\tskipped\n")
            continue
        tokens = []
        for pos, s, copy, column, kind, base in (tuple(int(v) for v in row) for row in edits[off[w]:off[w + 1]]):
            m = lists[w][s].decode() if isinstance(lists[w][s], bytes) else lists[w][s]
            change = f"{m[column]}>{'ACGT'[base]}" if kind == 0 else f"+{'ACGT'[base]}" if kind == 1 else f"-{'ACGT'[base]}"
            tokens.append(f"{m}#{copy}:{column}{change}@{pos}")
        out.append("\t".join([str(name), str(len(tokens))] + tokens) + "\n")
    return "".join(out).encode()


def with_segment_copies(sg: SparseGenotypes, ws: WindowStructure, segment: int) -> SparseGenotypes:
    """sg with fields[:, 3] (copies) replaced by the copies of segment `segment` of ws (Engine.window_structure over genotype_windows(sg) with
    which = sg.locus) and ratio by ws.ratio; everything else is sg's own.  Device operations only.  Engine.call_alleles(...) then calls that
    segment of a compound locus as it calls a plain locus."""
    if isinstance(segment, bool) or not isinstance(segment, (int, np.integer)) or not 0 <= segment < WS_MAX_SEGMENTS:
        raise MtrError(f"segment must be an integer in 0..{WS_MAX_SEGMENTS - 1}, got {segment!r}")
    if tuple(ws.seg.shape) != (int(sg.read.shape[0]), 4, 4):
        raise MtrError(f"the structure has {tuple(ws.seg.shape)} segment columns for {int(sg.read.shape[0])} rows")
    fields = sg.fields.clone()
    fields[:, 3] = ws.seg[:, segment, 2]
    return sg._replace(fields=fields, ratio=ws.ratio.clone())


def format_allele_consensus(loci, cons: AlleleConsensus) -> bytes:
    """The consensus of Engine.allele_consensus as text, one tab-separated line per CALLED allele in allele order: locus index, allele (0 or 1),
    members, aligned, skipped, the sequence's length, the sequence as letters ("." when it is empty), and the locus' motif as given.
    loci: what the genotype call was given, (left_flank, motif, right_flank) each; cons: allele_consensus' result (tensors or numpy)."""
    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    bmot = [v[1].encode() if isinstance(v[1], str) else bytes(v[1]) for v in loci]
    m = len(bmot)
    off, bases, bb = host(cons.off).reshape(-1), host(cons.bases).reshape(-1), host(cons.backbone_read).reshape(-1)
    if len(off) != 2 * m + 1 or len(bb) != 2 * m:
        raise MtrError(f"{len(bb)} alleles for {m} loci")
    members, aligned, skipped = host(cons.members).reshape(-1), host(cons.aligned).reshape(-1), host(cons.skipped).reshape(-1)
    letters = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for A in range(2 * m):
        if bb[A] < 0:
            continue
        lo, hi = int(off[A]), int(off[A + 1])
        seq = letters[bases[lo:hi]].tobytes() if hi > lo else b"."
        cols = [A // 2, A % 2, int(members[A]), int(aligned[A]), int(skipped[A]), hi - lo]
        out.append("\t".join(str(c) for c in cols).encode() + b"\t" + seq + b"\t" + bmot[A // 2] + b"\n")
    return b"".join(out)


def _motif_rows(mot: ReportMotifs):
    """the group table of a ReportMotifs (tensors or numpy) as host rows (motif bytes, motif_len, repeats, reads, copies, bases)"""
    def host(t):
        return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    off, motifs = host(mot.motif_off), host(mot.motifs).tobytes()
    cols = [host(c).tolist() for c in (mot.g_repeats, mot.g_reads, mot.g_copies, mot.g_bases)]
    return [(motifs[int(off[g]):int(off[g + 1])], int(off[g + 1] - off[g]), *(int(c[g]) for c in cols)) for g in range(len(off) - 1)]


def _format_motif_rows(rows) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\n" % r for r in rows)


def format_motifs(mot: ReportMotifs) -> bytes:
    """The catalogue as text: one line per group in group order, motif TAB motif_len TAB repeats TAB reads TAB copies TAB bases LF."""
    return _format_motif_rows(_motif_rows(mot))


class MotifCatalog:
    """A running motif catalogue over the batches of a walk, on the host (it is small: one row per motif).  add(mot) merges the group
    table of a batch's ReportMotifs into it, keyed by motif; the batches of a walk hold disjoint reads, so every column adds.  The
    order is that of first appearance.
        cat = MotifCatalog()
        for fa in eng.walk_fasta_device(buf, w):
            if len(fa.lens):
                eng.run(); cat.add(eng.report_motif_tensors())"""

    def __init__(self):
        self._rows = {}                                      # motif -> [repeats, reads, copies, bases], in insertion order

    def add(self, mot: ReportMotifs) -> "MotifCatalog":
        for motif, _, *cols in _motif_rows(mot):
            have = self._rows.setdefault(motif, [0, 0, 0, 0])
            for c, v in enumerate(cols):
                have[c] += v
        return self

    def rows(self):
        """[(motif bytes, motif_len, repeats, reads, copies, bases)] in the order of first appearance"""
        return [(m, len(m), *cols) for m, cols in self._rows.items()]

    def format(self) -> bytes:
        """rows() as format_motifs prints a batch's"""
        return _format_motif_rows(self.rows())

    def __len__(self):
        return len(self._rows)


def pack_read(codes: np.ndarray) -> np.ndarray:
    """one read in the device layout of include/mtr_hip.h ("the host's own packing"): len//16 + 4 words, first base in the
    top bits of word 0, zero behind the read"""
    n = len(codes)
    nw = n // 16 + 4
    padded = np.zeros(nw * 16, np.uint32)
    padded[:n] = codes
    shifts = (30 - 2 * np.arange(16, dtype=np.uint32)).astype(np.uint32)
    return np.bitwise_or.reduce(padded.reshape(nw, 16) << shifts, axis=1).astype(np.uint32)


def codes_from_str(s: str) -> np.ndarray:
    """ACGT/acgt -> 0..3 (reference handle_one_file.c:169-188); anything else raises like the reference exits."""
    lut = np.full(256, 255, np.uint8)
    for ch, v in zip("ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
        lut[ord(ch)] = v
    a = lut[np.frombuffer(s.encode(), np.uint8)]
    if (a == 255).any():
        bad = s[int(np.argmax(a == 255))]
        raise ValueError(f"Invalid character: {bad}")
    return a
