"""ctypes host binding of libsc_fqcount_hip.so and a Python mirror of the reference's fq-count operator.

Mirrors (reference tree):
  src/fq_count.nim:7-11    fq_count_header
  src/fq_count.nim:14      proc fq_count*(fastq: string, basename: bool, absolute: bool)
  src/utils/helpers.nim:200-224   output_header / get_absolute / output_w_fnames
  src/utils/helpers.nim:29-34     error_msg / quit_error

The counting itself always goes through the C ABI (include/sc_fqcount.h) into the HIP kernels; there is
no Python or CPU fallback here: if the shared library is missing or no GPU is visible the calls raise.

A process that also uses PyTorch: `import torch` BEFORE the first call of this module.  torch ships a libamdhip64 of its own; whichever
copy is loaded first serves both, and with two copies in one process a device pointer of one runtime means nothing to the other
(`scfq_synth_device` / `count_device` on a torch tensor then fail with SCFQ_EHIP).
"""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCFQ_LIB_OVERRIDE") or os.path.join(os.path.dirname(_HERE), "libsc_fqcount_hip.so")

SCFQ_QUAL_HIST = 0x1
SCFQ_STRUCT_CHECK = 0x2
SCFQ_TIMING = 0x4
SCFQ_PREV_IN_MEMORY = 0x8
SCFQ_HIST_EXACT = 0x10
SCFQ_WAIT_STREAM = 0x20
SCFQ_EOPEN, SCFQ_EGZ, SCFQ_EHIP, SCFQ_ERCCL, SCFQ_EARG, SCFQ_EIO, SCFQ_ENOMEM, SCFQ_ESPEC, SCFQ_EPIPE = -1, -2, -3, -4, -5, -6, -7, -8, -9
SCFQ_COMM_RCCL, SCFQ_COMM_TCP = 0, 1
COMM_ID_BYTES = 128
PARTIAL_WORDS = 32
HIST_WORDS = 4 * 256

EXPORTS = [
    "scfq_count_file", "scfq_count_buffer", "scfq_partial_buffer", "scfq_partial_identity",
    "scfq_partial_combine", "scfq_partial_finalize", "scfq_format_tsv", "scfq_strerror",
    "scfq_last_error_detail", "scfq_last_timing", "scfq_device_bytes_now", "scfq_device_bytes_high_water", "scfq_device_count", "scfq_shutdown",
    "scfq_debug_partial_simple", "scfq_synth_plan", "scfq_synth_host", "scfq_synth_device", "scfq_synth_locate",
    "scfq_debug_read_file", "scfq_debug_gz_resume", "scfq_debug_stream_ms", "scfq_debug_hist_stats",
    "scfq_index_lines", "scfq_dedup_buffer", "scfq_dedup_file", "scfq_dedup_error_detail", "scfq_stage_file",
    "scfq_device_free", "scfq_meta_header", "scfq_meta_file_tsv", "scfq_debug_bgzf_inflate",
    "scfq_set_wait_stream", "scfq_get_wait_stream", "scfq_count_file_sharded",
    "scfq_comm_unique_id", "scfq_comm_init_rank", "scfq_comm_init_rendezvous", "scfq_comm_init_all", "scfq_comm_world",
    "scfq_comm_rank", "scfq_comm_is_broken", "scfq_prepare", "scfq_comm_transport", "scfq_comm_exchange", "scfq_comm_exchange_start", "scfq_comm_exchange_finish",
    "scfq_comm_allgather_u64", "scfq_comm_destroy", "scfq_comm_error_detail", "scfq_debug_stages", "scfq_debug_stage_mark",
    "scfq_debug_gz_member_boundary", "scfq_debug_gz_shard_fix", "scfq_debug_last_scan_kernel", "scfq_debug_scan_geometry",
    "scfq_read_stats_buffer", "scfq_read_stats_file", "scfq_format_read_stats_tsv", "scfq_read_stats_error_detail",
    "scfq_debug_read_stats_stages",
    "scfq_cycles_buffer", "scfq_cycles_file", "scfq_format_cycle_row_tsv", "scfq_cycles_error_detail", "scfq_debug_cycles_stages",
    "scfq_kmers_buffer", "scfq_kmers_file", "scfq_format_kmer_tsv", "scfq_kmers_error_detail", "scfq_debug_kmers_stages",
    "scfq_adapters_buffer", "scfq_adapters_file", "scfq_adapters_default", "scfq_format_adapter_row_tsv", "scfq_adapters_error_detail",
    "scfq_debug_adapters_stages",
    "scfq_insert_size_buffers", "scfq_insert_size_files", "scfq_format_insert_size_tsv", "scfq_insert_size_error_detail",
    "scfq_debug_insert_size_stages",
    "scfq_merge_buffers", "scfq_merge_files", "scfq_format_merge_stats_tsv", "scfq_merge_error_detail", "scfq_debug_merge_stages",
    "scfq_trim_buffers", "scfq_trim_files", "scfq_format_trim_stats_tsv", "scfq_trim_error_detail", "scfq_debug_trim_stages",
    "scfq_screen_index_buffers", "scfq_screen_index_files", "scfq_screen_index_free", "scfq_screen_index_summary", "scfq_screen_ref_name",
    "scfq_screen_buffers", "scfq_screen_files", "scfq_format_screen_row_tsv", "scfq_screen_error_detail", "scfq_debug_screen_stages",
    "scfq_debug_screen_build_ms",
    "scfq_demux_sheet_new", "scfq_demux_sheet_free", "scfq_demux_sheet_samples", "scfq_demux_sheet_name", "scfq_demux_buffers", "scfq_demux_files",
    "scfq_format_demux_row_tsv", "scfq_demux_error_detail", "scfq_debug_demux_stages",
    "scfq_kcount_buffers", "scfq_kcount_files", "scfq_kcount_hist", "scfq_kcount_dump", "scfq_kcount_query", "scfq_kcount_free",
    "scfq_format_kcount_tsv", "scfq_kcount_error_detail", "scfq_debug_kcount_stages",
    "scfq_norm_buffers", "scfq_norm_files", "scfq_format_norm_row_tsv", "scfq_format_norm_hist_tsv", "scfq_norm_error_detail",
    "scfq_debug_norm_stages",
    "scfq_cplx_buffers", "scfq_cplx_files", "scfq_format_cplx_stats_tsv", "scfq_format_cplx_rec_tsv", "scfq_cplx_error_detail",
    "scfq_debug_cplx_stages",
    "scfq_rmdup_buffers", "scfq_rmdup_files", "scfq_format_rmdup_stats_tsv", "scfq_format_rmdup_rec_tsv", "scfq_rmdup_error_detail",
    "scfq_debug_rmdup_stages",
    "scfq_repair_buffers", "scfq_repair_files", "scfq_format_repair_stats_tsv", "scfq_format_repair_rec_tsv", "scfq_repair_error_detail",
    "scfq_debug_repair_stages",
    "scfq_fa_index_buffer", "scfq_fa_index_file", "scfq_fa_contig_at", "scfq_fa_contig_find", "scfq_fa_count_intervals",
    "scfq_fa_index_free", "scfq_fa_error_detail", "scfq_fa_parse_window", "scfq_fa_gc_interval", "scfq_format_fa_gc_value",
    "scfq_debug_fa_stages",
]


class Counts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "struct_size", "abi_version", "reads", "gc_bases", "n_bases", "bases", "lines", "newlines",
        "input_bytes", "bad_at", "bad_plus")] + [("qual_hist", ctypes.c_uint64 * 256)]


class Opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint64), ("n_devices", ctypes.c_int32),
                ("device_ids", ctypes.POINTER(ctypes.c_int32)), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("chunk_bytes", ctypes.c_uint64), ("wait_stream", ctypes.c_void_p)]


class Partial(ctypes.Structure):
    _fields_ = [("nl", ctypes.c_uint64), ("gc", ctypes.c_uint64 * 4), ("n", ctypes.c_uint64 * 4),
                ("len", ctypes.c_uint64 * 4), ("starts", ctypes.c_uint64 * 4),
                ("first_at", ctypes.c_uint64 * 4), ("first_plus", ctypes.c_uint64 * 4),
                ("bytes", ctypes.c_uint64), ("last_byte", ctypes.c_uint64), ("hist_class", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64 * 4)]

    def words(self):
        return list((ctypes.c_uint64 * PARTIAL_WORDS).from_buffer_copy(self))

    @classmethod
    def from_words(cls, w):
        arr = (ctypes.c_uint64 * PARTIAL_WORDS)(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in w])
        return cls.from_buffer_copy(arr)


class Timing(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint64), ("scan_kernel_ms", ctypes.c_double),
                ("fold_kernel_ms", ctypes.c_double), ("scan_bytes", ctypes.c_uint64),
                ("scan_launches", ctypes.c_uint64), ("host_fill_ms", ctypes.c_double),
                ("ingest_wall_ms", ctypes.c_double), ("h2d_bytes", ctypes.c_uint64), ("h2d_ms", ctypes.c_double)]


class DedupStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("struct_size", "total_reads", "duplicates", "false_positive", "records_out",
                                               "bytes_out", "hash_collisions")]


class ReadRec(ctypes.Structure):
    """scfq_read_rec: one row of the per-read table (five uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("seq_len", "gc_bases", "n_bases", "qual_len", "qual_sum")]


LEN_HIST_BINS, GC_HIST_BINS, MEANQ_HIST_BINS = 65, 102, 256


class ReadSummary(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "struct_size", "abi_version", "reads", "lines", "input_bytes", "bases", "gc_bases", "n_bases", "qual_bytes", "qual_sum",
        "min_len", "max_len", "n50", "l50", "n90", "l90")] + [
        ("len_hist", ctypes.c_uint64 * LEN_HIST_BINS), ("gc_hist", ctypes.c_uint64 * GC_HIST_BINS),
        ("meanq_hist", ctypes.c_uint64 * MEANQ_HIST_BINS), ("no_qual", ctypes.c_uint64)]


CYCLE_FIELDS = ("bases", "a", "c", "g", "t", "n", "quals", "qual_sum")
CYCLES_MAX_CAP = 1 << 24


class CycleRow(ctypes.Structure):
    """scfq_cycle_row: one position of the fq-cycles table (eight uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in CYCLE_FIELDS]


class CycleSummary(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("struct_size", "abi_version", "reads", "lines", "input_bytes", "max_seq_len", "max_qual_len",
                                               "cycles")] + [("tail", CycleRow), ("total", CycleRow)]


KMERS_MAX_K = 12
SCFQ_KMERS_CANONICAL = 0x1
KMER_SUMMARY_FIELDS = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "k", "flags", "windows", "kmers", "skipped",
                       "short_lines", "distinct", "max_count", "table_entries")


class KmerSummary(ctypes.Structure):
    """scfq_kmer_summary (fourteen uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in KMER_SUMMARY_FIELDS]


ADAPTERS_MAX_PROBES = 8
ADAPTERS_MAX_LEN = 32
ADAPTERS_MAX_CAP = 1 << 24
ADAPTER_SUMMARY_HEAD = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "n_probes", "max_seq_len", "positions")


class AdapterRow(ctypes.Structure):
    """scfq_adapter_row: one position of the fq-adapters table (nine uint64: first[8], any)"""
    _fields_ = [("first", ctypes.c_uint64 * ADAPTERS_MAX_PROBES), ("any", ctypes.c_uint64)]


class AdapterSummary(ctypes.Structure):
    """scfq_adapter_summary (42 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in ADAPTER_SUMMARY_HEAD] + \
               [("probe_len", ctypes.c_uint64 * ADAPTERS_MAX_PROBES), ("hits", ctypes.c_uint64 * ADAPTERS_MAX_PROBES),
                ("tail", AdapterRow), ("total", AdapterRow)]


INSERT_MAX_LEN = 512
INSERT_HIST_BINS = 1024
SCFQ_INSERT_INTERLEAVED = 0x1
INSERT_SUMMARY_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                         "overlapped", "not_overlapped", "too_long", "read_through", "overlap_bases", "mismatches", "insert_sum",
                         "insert_sq_sum", "min_insert", "max_insert", "mode_insert", "median_insert", "min_overlap", "max_mismatches",
                         "max_mismatch_pct")


class OverlapRec(ctypes.Structure):
    """scfq_overlap_rec: one pair of the fq-insert-size table (8 bytes)"""
    _fields_ = [("offset", ctypes.c_int32), ("overlap", ctypes.c_uint16), ("mismatches", ctypes.c_uint16)]


class InsertOpts(ctypes.Structure):
    """scfq_insert_opts"""
    _fields_ = [("struct_size", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("min_overlap", ctypes.c_uint32),
                ("max_mismatches", ctypes.c_uint32), ("max_mismatch_pct", ctypes.c_uint32)]


class InsertSummary(ctypes.Structure):
    """scfq_insert_summary (25 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in INSERT_SUMMARY_FIELDS]


SCFQ_MERGE_INTERLEAVED = 0x1
MERGE_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                      "merged", "not_overlapped", "too_long", "merged_bases", "overlap_bases", "mismatches", "took_mate1", "took_mate2",
                      "neither_valid", "merged_bytes", "unmerged1_bytes", "unmerged2_bytes", "min_overlap", "max_mismatches", "max_mismatch_pct",
                      "phred_offset")


class MergeOpts(ctypes.Structure):
    """scfq_merge_opts"""
    _fields_ = [("struct_size", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("min_overlap", ctypes.c_uint32),
                ("max_mismatches", ctypes.c_uint32), ("max_mismatch_pct", ctypes.c_uint32), ("phred_offset", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class MergeStats(ctypes.Structure):
    """scfq_merge_stats (26 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in MERGE_STATS_FIELDS]


SCFQ_TRIM_INTERLEAVED, SCFQ_TRIM_NO_OVERLAP, SCFQ_TRIM_NO_ADAPTERS = 0x1, 0x2, 0x4
SCFQ_TRIM_MAX_LEN, SCFQ_TRIM_MAX_PROBES = 512, 8
TRIM_PARAM_FIELDS = ("flags", "min_overlap", "max_mismatches", "max_mismatch_pct", "min_adapter_overlap", "adapter_mismatch_pct", "poly_g", "window",
                     "window_quality", "min_length", "phred_offset", "n_probes")
TRIM_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                     "reads_in", "reads_out", "too_long", "short_reads", "dropped_reads", "bases_in", "bases_out", "cut_overlap", "cut_adapter",
                     "cut_polyg", "cut_quality", "bases_overlap", "bases_adapter", "bases_polyg", "bases_quality", "adapter_reads", "bases_dropped",
                     "overlapped_pairs", "out1_bytes", "out2_bytes") + TRIM_PARAM_FIELDS


class TrimOpts(ctypes.Structure):
    """scfq_trim_opts (128 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in TRIM_PARAM_FIELDS] + \
               [("reserved", ctypes.c_uint32 * 2), ("probes", ctypes.c_char_p * 8)]


class TrimStats(ctypes.Structure):
    """scfq_trim_stats (49 uint64)"""
    _fields_ = [(n, ctypes.c_uint64 * 8 if n == "adapter_reads" else ctypes.c_uint64) for n in TRIM_STATS_FIELDS]


SCFQ_SCREEN_INTERLEAVED, SCFQ_SCREEN_KEEP_MATCHED = 0x1, 0x2
SCFQ_SCREEN_MAX_REFS, SCFQ_SCREEN_MAX_K, SCFQ_SCREEN_MAX_REF_BASES = 16, 32, 1 << 27
SCREEN_REF_FIELDS = ("contigs", "bases", "windows", "kmers", "distinct", "shared")
SCREEN_PER_REF_FIELDS = ("ref_reads", "ref_only_reads", "ref_best_reads", "ref_kmer_hits")
SCREEN_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                       "reads_in", "reads_out", "dropped_reads", "matched_reads", "matched_pairs", "multi_reads", "short_reads", "bases_in",
                       "bases_out", "windows", "kmers", "skipped", "hit_kmers") + SCREEN_PER_REF_FIELDS + \
                      ("out1_bytes", "out2_bytes", "flags", "min_hits", "min_hit_pct", "k", "n_refs")


class ScreenRef(ctypes.Structure):
    """scfq_screen_ref"""
    _fields_ = [("name", ctypes.c_char_p), ("text", ctypes.c_void_p), ("n", ctypes.c_uint64)]


class ScreenRefSummary(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in SCREEN_REF_FIELDS]


class ScreenSummary(ctypes.Structure):
    """scfq_screen_summary (6 + 16 x 6 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("struct_size", "abi_version", "n_refs", "k", "distinct", "slots")] + [("ref", ScreenRefSummary * 16)]


class ScreenOpts(ctypes.Structure):
    """scfq_screen_opts (24 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in ("flags", "min_hits", "min_hit_pct", "reserved")]


class ScreenRec(ctypes.Structure):
    """scfq_screen_rec (16 bytes)"""
    _fields_ = [("kmers", ctypes.c_uint32), ("hit_kmers", ctypes.c_uint32), ("best_hits", ctypes.c_uint32), ("mask", ctypes.c_uint16),
                ("best", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class ScreenStats(ctypes.Structure):
    """scfq_screen_stats (94 uint64)"""
    _fields_ = [(n, ctypes.c_uint64 * 16 if n in SCREEN_PER_REF_FIELDS else ctypes.c_uint64) for n in SCREEN_STATS_FIELDS]


SCFQ_DEMUX_INTERLEAVED, SCFQ_DEMUX_HEADER, SCFQ_DEMUX_KEEP_BARCODE = 0x1, 0x2, 0x4
SCFQ_DEMUX_ASSIGNED, SCFQ_DEMUX_UNMATCHED, SCFQ_DEMUX_AMBIGUOUS, SCFQ_DEMUX_NO_BARCODE = 0, 1, 2, 3
DEMUX_MAX_SAMPLES, DEMUX_MAX_BARCODE = 1024, 32
DEMUX_ROW_FIELDS = ("units", "perfect", "mismatched", "bases_out", "bytes1", "bytes2", "off1", "off2")
DEMUX_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                      "units_in", "assigned", "undetermined", "no_barcode", "unmatched", "ambiguous", "perfect", "mismatched", "reads_in", "reads_out",
                      "bases_in", "bases_out", "bases_clipped", "out1_bytes", "out2_bytes", "flags", "mismatches", "n_samples", "dual")


class DemuxSample(ctypes.Structure):
    """scfq_demux_sample"""
    _fields_ = [("name", ctypes.c_char_p), ("barcode1", ctypes.c_char_p), ("barcode2", ctypes.c_char_p)]


class DemuxOpts(ctypes.Structure):
    """scfq_demux_opts (24 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("mismatches", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class DemuxRow(ctypes.Structure):
    """scfq_demux_row (eight uint64): one destination"""
    _fields_ = [(n, ctypes.c_uint64) for n in DEMUX_ROW_FIELDS]


class DemuxRec(ctypes.Structure):
    """scfq_demux_rec (8 bytes): one unit"""
    _fields_ = [("sample", ctypes.c_uint16), ("mm1", ctypes.c_uint8), ("mm2", ctypes.c_uint8), ("state", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3)]


class DemuxStats(ctypes.Structure):
    """scfq_demux_stats (29 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in DEMUX_STATS_FIELDS]


SCFQ_EFULL = -10
SCFQ_KCOUNT_MIN_K, SCFQ_KCOUNT_MAX_K, SCFQ_KCOUNT_CANONICAL = 13, 32, 0x1
KCOUNT_SUMMARY_FIELDS = ("struct_size", "abi_version", "reads", "lines", "input_bytes", "k", "flags", "windows", "kmers", "skipped",
                         "short_lines", "distinct", "unique", "max_count", "slots", "passes")


class KcountOpts(ctypes.Structure):
    """scfq_kcount_opts (24 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64), ("k", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("table_bits", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class KcountSummary(ctypes.Structure):
    """scfq_kcount_summary (sixteen uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in KCOUNT_SUMMARY_FIELDS]


class KmerCount(ctypes.Structure):
    """scfq_kmer_count"""
    _fields_ = [("key", ctypes.c_uint64), ("count", ctypes.c_uint64)]


SCFQ_NORM_MAX_DEPTH = 0xFFFFFFFE
SCFQ_NORM_INTERLEAVED, SCFQ_NORM_KEEP_NO_KMERS = 0x1, 0x2
NORM_MAX_BINS = 1 << 20
NORM_REC_FIELDS = ("kmers", "depth", "min_count", "weak")
NORM_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                     "units_in", "units_out", "reads_in", "reads_out", "dropped_no_kmers", "dropped_low", "dropped_high", "short_reads",
                     "bases_in", "bases_out", "windows", "kmers", "skipped", "weak_kmers", "absent_kmers", "out1_bytes", "out2_bytes",
                     "flags", "k", "table_flags", "target", "min_depth", "weak_below", "seed", "distinct", "slots", "passes")


class NormOpts(ctypes.Structure):
    """scfq_norm_opts (48 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64)] + \
               [(n, ctypes.c_uint32) for n in ("flags", "k", "table_flags", "table_bits", "target", "min_depth", "weak_below", "reserved")] + \
               [("seed", ctypes.c_uint64)]


class NormRec(ctypes.Structure):
    """scfq_norm_rec (16 bytes)"""
    _fields_ = [(n, ctypes.c_uint32) for n in NORM_REC_FIELDS]


class NormStats(ctypes.Structure):
    """scfq_norm_stats (37 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in NORM_STATS_FIELDS]


SCFQ_CPLX_INTERLEAVED = 0x1
SCFQ_CPLX_MASK_NONE, SCFQ_CPLX_MASK_LOWER, SCFQ_CPLX_MASK_N = 0, 1, 2
SCFQ_CPLX_MAX_LEN, SCFQ_CPLX_SCORE_BINS = 512, 312
CPLX_MASKS = {"none": SCFQ_CPLX_MASK_NONE, "lower": SCFQ_CPLX_MASK_LOWER, "n": SCFQ_CPLX_MASK_N}
CPLX_PARAM_FIELDS = ("flags", "window", "threshold", "mask", "max_masked_pct")
CPLX_REC_FIELDS = ("score", "masked", "first", "intervals")
CPLX_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                     "reads_in", "reads_out", "too_long", "low_reads", "dropped_reads", "masked_reads", "perfect_intervals", "bases_in", "bases_out",
                     "masked_bases", "masked_bases_out", "max_score", "out1_bytes", "out2_bytes") + CPLX_PARAM_FIELDS
CPLX_REC_DTYPE = [(n, "<u2") for n in CPLX_REC_FIELDS]      # numpy: np.dtype(CPLX_REC_DTYPE), 8 bytes


class CplxOpts(ctypes.Structure):
    """scfq_cplx_opts (40 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in CPLX_PARAM_FIELDS] + [("reserved", ctypes.c_uint32 * 3)]


class CplxRec(ctypes.Structure):
    """scfq_cplx_rec (8 bytes)"""
    _fields_ = [(n, ctypes.c_uint16) for n in CPLX_REC_FIELDS]


class CplxStats(ctypes.Structure):
    """scfq_cplx_stats (29 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in CPLX_STATS_FIELDS]


SCFQ_RMDUP_INTERLEAVED, SCFQ_RMDUP_SWAPPED = 0x1, 0x2
SCFQ_RMDUP_HIST_BINS, SCFQ_RMDUP_MAX_PREFIX = 1025, 65535
RMDUP_PARAM_FIELDS = ("flags", "prefix", "hash_bits")
RMDUP_REC_FIELDS = ("rep", "copies")
RMDUP_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "unpaired",
                      "units_in", "units_out", "reads_in", "reads_out", "duplicate_units", "duplicated_classes", "max_copies", "bases_in", "bases_out",
                      "collisions", "rounds", "out1_bytes", "out2_bytes") + RMDUP_PARAM_FIELDS
RMDUP_REC_DTYPE = [(n, "<u4") for n in RMDUP_REC_FIELDS]      # numpy: np.dtype(RMDUP_REC_DTYPE), 8 bytes


class RmdupOpts(ctypes.Structure):
    """scfq_rmdup_opts (32 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in RMDUP_PARAM_FIELDS] + [("reserved", ctypes.c_uint32 * 3)]


class RmdupRec(ctypes.Structure):
    """scfq_rmdup_rec (8 bytes)"""
    _fields_ = [(n, ctypes.c_uint32) for n in RMDUP_REC_FIELDS]


class RmdupStats(ctypes.Structure):
    """scfq_rmdup_stats (26 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in RMDUP_STATS_FIELDS]


SCFQ_REPAIR_SINGLE = 0xFFFFFFFF
REPAIR_OUTPUTS = ("out1", "out2", "singles1", "singles2")
REPAIR_STATS_FIELDS = ("struct_size", "abi_version", "reads1", "reads2", "lines1", "lines2", "input_bytes1", "input_bytes2", "pairs", "singles1", "singles2",
                       "moved", "in_step", "repeated1", "repeated2", "collisions", "rounds", "path", "out1_bytes", "out2_bytes", "singles1_bytes",
                       "singles2_bytes", "flags", "hash_bits")
REPAIR_HASH_FIELDS = ("collisions", "rounds", "path")      # the three that depend on the hash or on the fast path


class RepairOpts(ctypes.Structure):
    """scfq_repair_opts (32 bytes)"""
    _fields_ = [("struct_size", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


class RepairStats(ctypes.Structure):
    """scfq_repair_stats (24 uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in REPAIR_STATS_FIELDS]


FA_SUMMARY_FIELDS = ("struct_size", "abi_version", "input_bytes", "tiles", "contigs", "bases", "gc_bases", "acgt_bases", "orphan_bases")


class FaSummary(ctypes.Structure):
    """scfq_fa_summary (nine uint64)"""
    _fields_ = [(n, ctypes.c_uint64) for n in FA_SUMMARY_FIELDS]


class FaContig(ctypes.Structure):
    """scfq_fa_contig: the name is owned by the index"""
    _fields_ = [("name", ctypes.c_char_p), ("name_len", ctypes.c_uint64), ("header_offset", ctypes.c_uint64), ("length", ctypes.c_uint64)]


class FaInterval(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("contig", "begin", "end")]


class FaCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("gc", "acgt", "bases")]


class SynthInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("struct_size", "records", "bytes", "gc_bases", "n_bases", "bases")]


class ScfqError(RuntimeError):
    def __init__(self, rc, what, detail=""):
        self.rc = rc
        super().__init__("%s failed: rc=%d (%s)%s" % (what, rc, strerror(rc), (" — " + detail) if detail else ""))


_lib = None


def lib():
    """Loads the HIP library; fails loudly when it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libsc_fqcount_hip.so not built: run `make -C %s` (hipcc --offload-arch=gfx950)"
                              % os.path.dirname(LIB_PATH))
        L = ctypes.CDLL(LIB_PATH)
        L.scfq_count_file.argtypes = [ctypes.c_char_p, ctypes.POINTER(Opts), ctypes.POINTER(Counts)]
        L.scfq_count_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(Opts),
                                        ctypes.POINTER(Counts)]
        L.scfq_partial_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(Opts), ctypes.POINTER(Partial), ctypes.c_void_p]
        L.scfq_partial_identity.argtypes = [ctypes.POINTER(Partial), ctypes.c_void_p]
        L.scfq_partial_identity.restype = None
        L.scfq_partial_combine.argtypes = [ctypes.POINTER(Partial), ctypes.POINTER(Partial), ctypes.c_void_p,
                                           ctypes.c_void_p]
        L.scfq_partial_finalize.argtypes = [ctypes.POINTER(Partial), ctypes.c_void_p, ctypes.POINTER(Counts)]
        L.scfq_format_tsv.argtypes = [ctypes.POINTER(Counts), ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_strerror.argtypes = [ctypes.c_int]
        L.scfq_strerror.restype = ctypes.c_char_p
        L.scfq_last_error_detail.restype = ctypes.c_char_p
        L.scfq_last_timing.argtypes = [ctypes.POINTER(Timing)]
        L.scfq_debug_partial_simple.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                ctypes.POINTER(Partial)]
        for name in ("scfq_synth_plan",):
            getattr(L, name).argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                         ctypes.POINTER(SynthInfo)]
        for name in ("scfq_synth_host", "scfq_synth_device"):
            getattr(L, name).argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(SynthInfo)]
        L.scfq_debug_read_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
        L.scfq_debug_read_file.restype = ctypes.c_int64
        L.scfq_debug_gz_resume.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
        L.scfq_debug_gz_resume.restype = ctypes.c_int64
        L.scfq_dedup_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(DedupStats)]
        L.scfq_dedup_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(DedupStats)]
        L.scfq_dedup_error_detail.restype = ctypes.c_char_p
        L.scfq_stage_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_uint64)]
        L.scfq_device_free.argtypes = [ctypes.c_void_p]
        L.scfq_meta_header.restype = ctypes.c_char_p
        L.scfq_meta_file_tsv.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_debug_bgzf_inflate.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
        L.scfq_debug_bgzf_inflate.restype = ctypes.c_int64
        L.scfq_index_lines.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.POINTER(ctypes.c_uint64)]
        L.scfq_debug_stream_ms.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
        L.scfq_debug_stream_ms.restype = ctypes.c_double
        L.scfq_synth_locate.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.scfq_set_wait_stream.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.scfq_get_wait_stream.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.scfq_get_wait_stream.restype = ctypes.c_void_p
        vp, pvp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
        L.scfq_comm_unique_id.argtypes = [vp, ctypes.c_uint64]
        L.scfq_comm_init_rank.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, pvp]
        L.scfq_comm_init_rendezvous.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, pvp]
        L.scfq_comm_init_all.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, pvp]
        L.scfq_comm_world.argtypes = [vp]
        L.scfq_comm_rank.argtypes = [vp]
        L.scfq_device_bytes_now.restype = ctypes.c_uint64
        L.scfq_device_bytes_high_water.restype = ctypes.c_uint64
        L.scfq_comm_is_broken.argtypes = [vp]
        L.scfq_prepare.argtypes = [ctypes.POINTER(Opts)]
        L.scfq_comm_transport.argtypes = [vp]
        L.scfq_comm_transport.restype = ctypes.c_char_p
        L.scfq_comm_exchange.argtypes = [vp, ctypes.POINTER(Partial), vp, ctypes.POINTER(Partial), vp, ctypes.c_int]
        L.scfq_comm_exchange_start.argtypes = [vp, ctypes.POINTER(Partial), vp, ctypes.c_int]
        L.scfq_comm_exchange_finish.argtypes = [vp, ctypes.POINTER(Partial), vp, ctypes.c_int]
        L.scfq_comm_allgather_u64.argtypes = [vp, vp, ctypes.c_uint32, vp, ctypes.c_int]
        L.scfq_comm_destroy.argtypes = [vp]
        L.scfq_comm_error_detail.restype = ctypes.c_char_p
        L.scfq_count_file_sharded.argtypes = [ctypes.c_char_p, ctypes.POINTER(Opts), vp, ctypes.POINTER(Counts)]
        L.scfq_read_stats_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.POINTER(ReadSummary)]
        L.scfq_read_stats_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ReadSummary)]
        L.scfq_format_read_stats_tsv.argtypes = [ctypes.POINTER(ReadSummary), ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_read_stats_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_read_stats_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_cycles_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.POINTER(CycleSummary)]
        L.scfq_cycles_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(CycleSummary)]
        L.scfq_format_cycle_row_tsv.argtypes = [ctypes.POINTER(CycleRow), ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_cycles_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_cycles_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_kmers_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                        ctypes.c_uint64, ctypes.POINTER(KmerSummary)]
        L.scfq_kmers_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.POINTER(KmerSummary)]
        L.scfq_format_kmer_tsv.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_kmers_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_kmers_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_adapters_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(AdapterSummary)]
        L.scfq_adapters_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.POINTER(AdapterSummary)]
        L.scfq_adapters_default.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p)]
        L.scfq_format_adapter_row_tsv.argtypes = [ctypes.POINTER(AdapterRow), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p,
                                                  ctypes.c_uint64]
        L.scfq_adapters_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_adapters_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_insert_size_buffers.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                               ctypes.POINTER(InsertOpts), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.POINTER(InsertSummary)]
        L.scfq_insert_size_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(InsertOpts), ctypes.c_void_p,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(InsertSummary)]
        L.scfq_format_insert_size_tsv.argtypes = [ctypes.POINTER(InsertSummary), ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_insert_size_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_insert_size_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_merge_buffers.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(MergeOpts),
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.c_int, ctypes.POINTER(MergeStats)]
        L.scfq_merge_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(MergeOpts), ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(MergeStats)]
        L.scfq_format_merge_stats_tsv.argtypes = [ctypes.POINTER(MergeStats), ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_merge_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_merge_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_trim_buffers.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(TrimOpts),
                                        ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(TrimStats)]
        L.scfq_trim_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(TrimOpts), ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(TrimStats)]
        L.scfq_format_trim_stats_tsv.argtypes = [ctypes.POINTER(TrimStats), ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_trim_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_trim_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_screen_index_buffers.argtypes = [ctypes.POINTER(ScreenRef), ctypes.c_uint32, ctypes.c_uint32, pvp, ctypes.POINTER(ScreenSummary)]
        L.scfq_screen_index_files.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_void_p, pvp, ctypes.POINTER(ScreenSummary)]
        L.scfq_screen_index_free.argtypes = [vp]
        L.scfq_screen_index_free.restype = None
        L.scfq_screen_index_summary.argtypes = [vp, ctypes.POINTER(ScreenSummary)]
        L.scfq_screen_ref_name.argtypes = [vp, ctypes.c_uint32]
        L.scfq_screen_ref_name.restype = ctypes.c_char_p
        L.scfq_screen_buffers.argtypes = [vp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ScreenOpts),
                                          ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                          ctypes.c_int, ctypes.POINTER(ScreenStats)]
        L.scfq_screen_files.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ScreenOpts), ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ScreenStats)]
        L.scfq_format_screen_row_tsv.argtypes = [ctypes.POINTER(ScreenStats), vp, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_screen_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_screen_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_debug_screen_build_ms.argtypes = [vp]
        L.scfq_debug_screen_build_ms.restype = ctypes.c_double
        L.scfq_demux_sheet_new.argtypes = [ctypes.POINTER(DemuxSample), ctypes.c_uint32, pvp]
        L.scfq_demux_sheet_free.argtypes = [vp]
        L.scfq_demux_sheet_free.restype = None
        L.scfq_demux_sheet_samples.argtypes = [vp]
        L.scfq_demux_sheet_samples.restype = ctypes.c_uint32
        L.scfq_demux_sheet_name.argtypes = [vp, ctypes.c_uint32]
        L.scfq_demux_sheet_name.restype = ctypes.c_char_p
        L.scfq_demux_buffers.argtypes = [vp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(DemuxOpts),
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(DemuxStats)]
        L.scfq_demux_files.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(DemuxOpts), ctypes.c_char_p, ctypes.c_void_p,
                                       ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(DemuxStats)]
        L.scfq_format_demux_row_tsv.argtypes = [ctypes.POINTER(DemuxStats), vp, ctypes.c_uint32, ctypes.POINTER(DemuxRow), ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_demux_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_demux_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_kcount_buffers.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_int, vp, pvp, vp]
        L.scfq_kcount_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, vp, vp, pvp, vp]
        L.scfq_kcount_hist.argtypes = [vp, vp, ctypes.c_uint64]
        L.scfq_kcount_dump.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.scfq_kcount_query.argtypes = [vp, vp, ctypes.c_uint64, vp]
        L.scfq_kcount_free.argtypes = [vp]
        L.scfq_kcount_free.restype = None
        L.scfq_format_kcount_tsv.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_kcount_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_kcount_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_norm_buffers.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_int, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp,
                                        ctypes.c_uint64, ctypes.c_int, vp, ctypes.c_uint64, vp]
        L.scfq_norm_files.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp]
        L.scfq_format_norm_row_tsv.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_format_norm_hist_tsv.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_norm_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_norm_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_cplx_buffers.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_int, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp,
                                        ctypes.c_uint64, ctypes.c_int, vp]
        L.scfq_cplx_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
        L.scfq_format_cplx_stats_tsv.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_format_cplx_rec_tsv.argtypes = [ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_cplx_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_cplx_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_rmdup_buffers.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_int, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp,
                                         ctypes.c_uint64, ctypes.c_int, vp]
        L.scfq_rmdup_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
        L.scfq_format_rmdup_stats_tsv.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_format_rmdup_rec_tsv.argtypes = [ctypes.c_uint64, vp, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_rmdup_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_rmdup_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_repair_buffers.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64, ctypes.c_int, vp, vp, ctypes.c_uint64] + [vp, ctypes.c_uint64] * 4 + [
            ctypes.c_int, vp]
        L.scfq_repair_files.argtypes = [ctypes.c_char_p, ctypes.c_char_p, vp, vp] + [ctypes.c_int] * 5 + [vp]
        L.scfq_format_repair_stats_tsv.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_format_repair_rec_tsv.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_repair_error_detail.restype = ctypes.c_char_p
        L.scfq_debug_repair_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        L.scfq_fa_index_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, pvp, ctypes.POINTER(FaSummary)]
        L.scfq_fa_index_file.argtypes = [ctypes.c_char_p, ctypes.c_void_p, pvp, ctypes.POINTER(FaSummary)]
        L.scfq_fa_contig_at.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(FaContig)]
        L.scfq_fa_contig_find.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
        L.scfq_fa_count_intervals.argtypes = [vp, vp, ctypes.c_uint64, vp]
        L.scfq_fa_index_free.argtypes = [vp]
        L.scfq_fa_index_free.restype = None
        L.scfq_fa_error_detail.restype = ctypes.c_char_p
        L.scfq_fa_parse_window.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
        L.scfq_fa_gc_interval.argtypes = [ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
        L.scfq_format_fa_gc_value.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
        L.scfq_debug_fa_stages.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_uint32]
        _lib = L
    return _lib


def strerror(rc):
    return lib().scfq_strerror(rc).decode()


def _check(rc, what):
    if rc != 0:
        raise ScfqError(rc, what, lib().scfq_last_error_detail().decode())


def make_opts(flags=0, devices=None, chunk_bytes=0, wait_stream=None):
    o = Opts()
    o.struct_size = ctypes.sizeof(Opts)
    o.flags = flags
    o.chunk_bytes = chunk_bytes
    if wait_stream is not None:          # 0 names the legacy default stream (what torch uses unless told otherwise)
        o.flags |= SCFQ_WAIT_STREAM
        o.wait_stream = wait_stream or None
    if devices:
        arr = (ctypes.c_int32 * len(devices))(*devices)
        o._keep = arr
        o.n_devices = len(devices)
        o.device_ids = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))
    return o


def _new_counts():
    c = Counts()
    c.struct_size = ctypes.sizeof(Counts)
    return c


def _host_ptr(data):
    """bytes / bytearray / numpy uint8 array -> (address, length, keepalive)"""
    if isinstance(data, (bytes, bytearray)):
        buf = (ctypes.c_char * len(data)).from_buffer_copy(data) if len(data) else (ctypes.c_char * 1)()
        return ctypes.addressof(buf), len(data), buf
    import numpy as np
    a = np.ascontiguousarray(data, dtype=np.uint8)
    return a.ctypes.data, a.size, a


def count_file(path, flags=0, devices=None, chunk_bytes=0):
    c = _new_counts()
    o = make_opts(flags, devices, chunk_bytes)
    _check(lib().scfq_count_file(os.fsencode(path), ctypes.byref(o), ctypes.byref(c)), "scfq_count_file")
    return c


def count_host(data, flags=0, devices=None, chunk_bytes=0):
    addr, n, keep = _host_ptr(data)
    c = _new_counts()
    o = make_opts(flags, devices, chunk_bytes)
    _check(lib().scfq_count_buffer(addr, n, 0, ctypes.byref(o), ctypes.byref(c)), "scfq_count_buffer")
    return c


def count_device(dev_ptr, n, flags=0, wait_stream=None):
    """wait_stream: hipStream_t (int) of the producer of the buffer, e.g. torch.cuda.current_stream().cuda_stream; None = the
    caller has synchronised (include/sc_fqcount.h: scfq_opts.wait_stream)"""
    c = _new_counts()
    o = make_opts(flags, wait_stream=wait_stream)
    _check(lib().scfq_count_buffer(ctypes.c_void_p(dev_ptr), n, 1, ctypes.byref(o), ctypes.byref(c)),
           "scfq_count_buffer")
    return c


def partial_device(dev_ptr, n, prev_byte=-1, flags=0, want_hist=False, wait_stream=None):
    p = Partial()
    o = make_opts(flags, wait_stream=wait_stream)
    hist = (ctypes.c_uint64 * HIST_WORDS)() if want_hist else None
    _check(lib().scfq_partial_buffer(ctypes.c_void_p(dev_ptr), n, 1, prev_byte, ctypes.byref(o), ctypes.byref(p),
                                     ctypes.byref(hist) if want_hist else None), "scfq_partial_buffer")
    return (p, hist) if want_hist else p


def partial_host(data, prev_byte=-1, flags=0, want_hist=False, chunk_bytes=0):
    addr, n, keep = _host_ptr(data)
    p = Partial()
    o = make_opts(flags, None, chunk_bytes)
    hist = (ctypes.c_uint64 * HIST_WORDS)() if want_hist else None
    _check(lib().scfq_partial_buffer(addr, n, 0, prev_byte, ctypes.byref(o), ctypes.byref(p),
                                     ctypes.byref(hist) if want_hist else None), "scfq_partial_buffer")
    return (p, hist) if want_hist else p


def set_wait_stream(stream):
    """this thread's default caller stream for device-pointer calls (scfq_set_wait_stream): an int hipStream_t handle
    (0 = the legacy default stream, e.g. torch.cuda.current_stream().cuda_stream); None clears it"""
    lib().scfq_set_wait_stream(ctypes.c_void_p(stream or 0), 0 if stream is None else 1)


class Comm:
    """scfq_comm: the cross-rank exchange of shard partials inside the C library (RCCL all-gather + rank-ordered fold)"""

    def __init__(self, handle):
        self.h = ctypes.c_void_p(handle)

    @staticmethod
    def _err(rc, what):
        if rc != 0:
            raise ScfqError(rc, what, lib().scfq_comm_error_detail().decode())

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        Comm._err(lib().scfq_comm_unique_id(buf, COMM_ID_BYTES), "scfq_comm_unique_id")
        return buf.raw

    @classmethod
    def init_rank(cls, uid, world, rank, device, timeout_ms=0):
        h = ctypes.c_void_p()
        cls._err(lib().scfq_comm_init_rank(uid, world, rank, device, timeout_ms, ctypes.byref(h)), "scfq_comm_init_rank")
        return cls(h.value)

    @classmethod
    def init_rendezvous(cls, host, port, world, rank, device=0, transport=SCFQ_COMM_RCCL, timeout_ms=0):
        h = ctypes.c_void_p()
        cls._err(lib().scfq_comm_init_rendezvous(host.encode() if host else None, port, world, rank, device, transport,
                                                 timeout_ms, ctypes.byref(h)), "scfq_comm_init_rendezvous")
        return cls(h.value)

    @classmethod
    def init_all(cls, devices, timeout_ms=0):
        n = len(devices)
        arr = (ctypes.c_int32 * n)(*devices)
        hs = (ctypes.c_void_p * n)()
        cls._err(lib().scfq_comm_init_all(n, arr, timeout_ms, hs), "scfq_comm_init_all")
        return [cls(h) for h in hs]

    world = property(lambda self: lib().scfq_comm_world(self.h))
    rank = property(lambda self: lib().scfq_comm_rank(self.h))
    transport = property(lambda self: lib().scfq_comm_transport(self.h).decode())
    broken = property(lambda self: bool(lib().scfq_comm_is_broken(self.h)))

    def exchange(self, partial, hist=None, timeout_ms=0):
        out = Partial()
        out_h = (ctypes.c_uint64 * HIST_WORDS)() if hist is not None else None
        self._err(lib().scfq_comm_exchange(self.h, ctypes.byref(partial), ctypes.byref(hist) if hist is not None else None,
                                           ctypes.byref(out), ctypes.byref(out_h) if hist is not None else None, timeout_ms),
                  "scfq_comm_exchange")
        return (out, out_h) if hist is not None else out

    def start(self, partial, hist=None, timeout_ms=0):
        self._err(lib().scfq_comm_exchange_start(self.h, ctypes.byref(partial), ctypes.byref(hist) if hist is not None else None,
                                                 timeout_ms), "scfq_comm_exchange_start")

    def finish(self, want_hist=False, timeout_ms=0):
        out = Partial()
        out_h = (ctypes.c_uint64 * HIST_WORDS)() if want_hist else None
        self._err(lib().scfq_comm_exchange_finish(self.h, ctypes.byref(out), ctypes.byref(out_h) if want_hist else None, timeout_ms),
                  "scfq_comm_exchange_finish")
        return (out, out_h) if want_hist else out

    def allgather_u64(self, words, timeout_ms=0):
        n = len(words)
        mine = (ctypes.c_uint64 * n)(*[int(w) & 0xFFFFFFFFFFFFFFFF for w in words])
        out = (ctypes.c_uint64 * (n * self.world))()
        self._err(lib().scfq_comm_allgather_u64(self.h, mine, n, out, timeout_ms), "scfq_comm_allgather_u64")
        return [list(out[r * n:(r + 1) * n]) for r in range(self.world)]

    def count_file(self, path, flags=0, devices=None, chunk_bytes=0):
        """scfq_count_file_sharded: this rank's byte range of `path`, exchange, the whole file's counters on every rank"""
        c = _new_counts()
        o = make_opts(flags, devices, chunk_bytes)
        _check(lib().scfq_count_file_sharded(os.fsencode(path), ctypes.byref(o), self.h, ctypes.byref(c)), "scfq_count_file_sharded")
        return c

    def destroy(self):
        if self.h:
            lib().scfq_comm_destroy(self.h)
            self.h = ctypes.c_void_p()


def index_lines_device(dev_ptr, n, line_off_ptr=None, cap=0):
    """K5: number of lines; with a device buffer of `cap` uint64 entries also writes the line-start offsets + sentinel"""
    lines = ctypes.c_uint64()
    _check(lib().scfq_index_lines(ctypes.c_void_p(dev_ptr), n, ctypes.c_void_p(line_off_ptr) if line_off_ptr else None, cap,
                                  ctypes.byref(lines)), "scfq_index_lines")
    return lines.value


def _new_dedup_stats():
    st = DedupStats()
    st.struct_size = ctypes.sizeof(DedupStats)
    return st


def dedup_device(dev_ptr, n, out_dev_ptr=None, out_cap=0):
    """fq-dedup of a device-resident FASTQ; result into device memory (out_dev_ptr None: size + statistics only).
    Returns (bytes_out, DedupStats)."""
    st = _new_dedup_stats()
    nb = ctypes.c_uint64()
    _check(lib().scfq_dedup_buffer(ctypes.c_void_p(dev_ptr), n, 1, ctypes.c_void_p(out_dev_ptr) if out_dev_ptr else None,
                                   out_cap, 1, ctypes.byref(nb), ctypes.byref(st)), "scfq_dedup_buffer")
    return nb.value, st


def dedup_host(data):
    """fq-dedup of a host buffer (bytes / numpy uint8); returns (bytes, DedupStats)"""
    addr, n, keep = _host_ptr(data)
    st = _new_dedup_stats()
    nb = ctypes.c_uint64()
    _check(lib().scfq_dedup_buffer(addr, n, 0, None, 0, 0, ctypes.byref(nb), ctypes.byref(st)), "scfq_dedup_buffer")
    out = (ctypes.c_uint8 * max(nb.value, 1))()
    st = _new_dedup_stats()
    _check(lib().scfq_dedup_buffer(addr, n, 0, out, nb.value, 0, ctypes.byref(nb), ctypes.byref(st)), "scfq_dedup_buffer")
    return bytes(out[:nb.value]), st


def dedup_file(path, out_fd=-1):
    st = _new_dedup_stats()
    _check(lib().scfq_dedup_file(os.fsencode(path), None, out_fd, ctypes.byref(st)), "scfq_dedup_file")
    return st


def _new_read_summary():
    s = ReadSummary()
    s.struct_size = ctypes.sizeof(ReadSummary)
    return s


def _check_read_stats(rc, what):
    if rc != 0:
        raise ScfqError(rc, what, lib().scfq_read_stats_error_detail().decode() or lib().scfq_last_error_detail().decode())


def read_stats_device(dev_ptr, n, records_ptr=None, cap=0):
    """fq-readstats of a device-resident FASTQ; records_ptr: device memory for `cap` ReadRec rows (None: summary only; size
    it with the `reads` of a summary-only call).  Returns the ReadSummary."""
    s = _new_read_summary()
    _check_read_stats(lib().scfq_read_stats_buffer(ctypes.c_void_p(dev_ptr), n, 1, ctypes.c_void_p(records_ptr) if records_ptr else None,
                                                   cap, ctypes.byref(s)), "scfq_read_stats_buffer")
    return s


def read_stats_host(data):
    """fq-readstats of a host buffer (bytes / numpy uint8); returns the ReadSummary"""
    addr, n, keep = _host_ptr(data)
    s = _new_read_summary()
    _check_read_stats(lib().scfq_read_stats_buffer(addr, n, 0, None, 0, ctypes.byref(s)), "scfq_read_stats_buffer")
    return s


def read_stats_file(path):
    s = _new_read_summary()
    _check_read_stats(lib().scfq_read_stats_file(os.fsencode(path), None, ctypes.byref(s)), "scfq_read_stats_file")
    return s


def format_read_stats_tsv(s):
    buf = ctypes.create_string_buffer(512)
    lib().scfq_format_read_stats_tsv(ctypes.byref(s), buf, 512)
    return buf.value.decode()


def read_stats_stages():
    """(index, R1, R2 sums + histograms, R2 N50 / N90) milliseconds of this thread's last read_stats call; the last three are HIP-event
    times and zeros unless SCFQ_READSTATS_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_read_stats_stages(ms, 4)
    return list(ms)


def _new_cycle_summary():
    s = CycleSummary()
    s.struct_size = ctypes.sizeof(CycleSummary)
    return s


def _cycles_call(fn, what, cap, *head):
    """rows: a caller's int64 array of shape (cap, 8) is filled in place ([cycles, cap) untouched) when `cap` is one"""
    import numpy as np
    if isinstance(cap, np.ndarray):
        buf = cap
        assert buf.dtype == np.int64 and buf.ndim == 2 and buf.shape[1] == 8 and buf.flags.c_contiguous
    else:
        buf = np.zeros((cap, 8), dtype=np.int64)
    s = _new_cycle_summary()
    rc = fn(*head, ctypes.c_void_p(buf.ctypes.data) if buf.shape[0] else None, buf.shape[0], ctypes.byref(s))
    if rc != 0:
        raise ScfqError(rc, what, lib().scfq_cycles_error_detail().decode() or lib().scfq_last_error_detail().decode())
    return s, buf[:s.cycles]


def cycles_device(dev_ptr, n, cap=0):
    """fq-cycles of a device-resident FASTQ, at most `cap` positions (0: the sizing call; read max_seq_len / max_qual_len).
    Returns (CycleSummary, rows as an int64 array of shape (cycles, 8), columns CYCLE_FIELDS)."""
    return _cycles_call(lib().scfq_cycles_buffer, "scfq_cycles_buffer", cap, ctypes.c_void_p(dev_ptr), n, 1)


def cycles_host(data, cap=0):
    """fq-cycles of a host buffer (bytes / numpy uint8)"""
    addr, n, keep = _host_ptr(data)
    return _cycles_call(lib().scfq_cycles_buffer, "scfq_cycles_buffer", cap, addr, n, 0)


def cycles_file(path, cap=0):
    return _cycles_call(lib().scfq_cycles_file, "scfq_cycles_file", cap, os.fsencode(path), None)


def format_cycle_row_tsv(row):
    """row: a CycleRow or eight integers in the order of CYCLE_FIELDS"""
    if not isinstance(row, CycleRow):
        row = CycleRow(*[int(v) for v in row])
    buf = ctypes.create_string_buffer(512)
    lib().scfq_format_cycle_row_tsv(ctypes.byref(row), buf, 512)
    return buf.value.decode()


def cycles_stages():
    """(index, line pass, counting kernel, finish) milliseconds of this thread's last cycles call; the last three are HIP-event
    times and zeros unless SCFQ_CYCLES_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_cycles_stages(ms, 4)
    return list(ms)


def _new_kmer_summary():
    s = KmerSummary()
    s.struct_size = ctypes.sizeof(KmerSummary)
    return s


def _kmers_call(fn, what, k, flags, table, *head):
    """table: None (the sizing and summary call), True (a fresh table of 4^k entries) or a caller's contiguous uint64 array of
    `cap` entries, filled in place ([4^k, cap) untouched)"""
    import numpy as np
    if table is True:
        table = np.zeros(4 ** k if 1 <= k <= KMERS_MAX_K else 1, dtype=np.uint64)
    if table is not None:
        assert isinstance(table, np.ndarray) and table.dtype == np.uint64 and table.ndim == 1 and table.flags.c_contiguous
    cap = 0 if table is None else table.shape[0]
    s = _new_kmer_summary()
    rc = fn(*head, k, flags, ctypes.c_void_p(table.ctypes.data) if cap else None, cap, ctypes.byref(s))
    if rc != 0:
        raise ScfqError(rc, what, lib().scfq_kmers_error_detail().decode() or lib().scfq_last_error_detail().decode())
    return s, (None if table is None else table[:s.table_entries])


def kmers_device(dev_ptr, n, k, flags=0, table=None):
    """fq-kmers of a device-resident FASTQ.  table: None (the sizing and summary call), True (a fresh table) or a uint64 array
    of at least 4^k entries.  Returns (KmerSummary, the 4^k entries as a uint64 array or None)."""
    return _kmers_call(lib().scfq_kmers_buffer, "scfq_kmers_buffer", k, flags, table, ctypes.c_void_p(dev_ptr), n, 1)


def kmers_host(data, k, flags=0, table=None):
    """fq-kmers of a host buffer (bytes / numpy uint8)"""
    addr, n, keep = _host_ptr(data)
    return _kmers_call(lib().scfq_kmers_buffer, "scfq_kmers_buffer", k, flags, table, addr, n, 0)


def kmers_file(path, k, flags=0, table=None):
    return _kmers_call(lib().scfq_kmers_file, "scfq_kmers_file", k, flags, table, os.fsencode(path), None)


def format_kmer_tsv(k, index, count):
    """"ACGT\\t12": the k letters of `index` and the count"""
    buf = ctypes.create_string_buffer(64)
    _check(min(0, lib().scfq_format_kmer_tsv(k, index, count, buf, 64)), "scfq_format_kmer_tsv")
    return buf.value.decode()


def kmers_stages():
    """(index, counting kernel, finish, copies to the host) milliseconds of this thread's last kmers call; the last three are
    HIP-event times and zeros unless SCFQ_KMERS_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_kmers_stages(ms, 4)
    return list(ms)


def _new_adapter_summary():
    s = AdapterSummary()
    s.struct_size = ctypes.sizeof(AdapterSummary)
    return s


def adapters_default():
    """the built-in probes as a list of (name, sequence)"""
    out, i = [], 0
    name, seq = ctypes.c_char_p(), ctypes.c_char_p()
    while lib().scfq_adapters_default(i, ctypes.byref(name), ctypes.byref(seq)) > 0:
        out.append((name.value.decode(), seq.value.decode()))
        i += 1
    return out


def _probe_array(probes):
    """probes: None (the built-in set) or a sequence of str / bytes"""
    if probes is None:
        probes = [seq for _, seq in adapters_default()]
    enc = [p.encode() if isinstance(p, str) else p for p in probes]
    return (ctypes.c_char_p * max(len(enc), 1))(*enc), len(enc)


def _adapters_call(fn, what, probes, cap, *head):
    """cap: the number of rows, or a caller's uint64 array of shape (cap, 9), filled in place ([positions, cap) untouched)"""
    import numpy as np
    if isinstance(cap, np.ndarray):
        buf = cap
        assert buf.dtype == np.uint64 and buf.ndim == 2 and buf.shape[1] == 9 and buf.flags.c_contiguous
    else:
        buf = np.zeros((cap, 9), dtype=np.uint64)
    arr, n_probes = _probe_array(probes)
    s = _new_adapter_summary()
    rc = fn(*head, arr, n_probes, ctypes.c_void_p(buf.ctypes.data) if buf.shape[0] else None, buf.shape[0], ctypes.byref(s))
    if rc != 0:
        raise ScfqError(rc, what, lib().scfq_adapters_error_detail().decode() or lib().scfq_last_error_detail().decode())
    return s, (buf[:s.positions] if buf.shape[0] else None)


def adapters_device(dev_ptr, n, probes=None, cap=0):
    """fq-adapters of a device-resident FASTQ, at most `cap` positions (0: the sizing call; read max_seq_len).  probes: None for the
    built-in set.  Returns (AdapterSummary, rows as a uint64 array of shape (positions, 9): first[0 .. 8) and any; None for cap 0)."""
    return _adapters_call(lib().scfq_adapters_buffer, "scfq_adapters_buffer", probes, cap, ctypes.c_void_p(dev_ptr), n, 1)


def adapters_host(data, probes=None, cap=0):
    """fq-adapters of a host buffer (bytes / numpy uint8)"""
    addr, n, keep = _host_ptr(data)
    return _adapters_call(lib().scfq_adapters_buffer, "scfq_adapters_buffer", probes, cap, addr, n, 0)


def adapters_file(path, probes=None, cap=0):
    return _adapters_call(lib().scfq_adapters_file, "scfq_adapters_file", probes, cap, os.fsencode(path), None)


def format_adapter_row_tsv(row, n_probes, reads, counts=False):
    """row: an AdapterRow or nine integers (first[0 .. 8), any)"""
    if not isinstance(row, AdapterRow):
        v = [int(x) for x in row]
        row = AdapterRow((ctypes.c_uint64 * ADAPTERS_MAX_PROBES)(*v[:8]), v[8])
    buf = ctypes.create_string_buffer(1024)
    _check(min(0, lib().scfq_format_adapter_row_tsv(ctypes.byref(row), n_probes, reads, 1 if counts else 0, buf, 1024)), "scfq_format_adapter_row_tsv")
    return buf.value.decode()


def adapters_stages():
    """(index, matching kernel, rows, finish) milliseconds of this thread's last adapters call; the last three are HIP-event times
    and zeros unless SCFQ_ADAPTERS_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_adapters_stages(ms, 4)
    return list(ms)


def _new_insert_summary():
    s = InsertSummary()
    s.struct_size = ctypes.sizeof(InsertSummary)
    return s


def insert_opts(interleaved=False, min_overlap=30, max_mismatches=5, max_mismatch_pct=20):
    o = InsertOpts()
    o.struct_size = ctypes.sizeof(InsertOpts)
    o.flags = SCFQ_INSERT_INTERLEAVED if interleaved else 0
    o.min_overlap, o.max_mismatches, o.max_mismatch_pct = min_overlap, max_mismatches, max_mismatch_pct
    return o


def _insert_call(fn, what, params, interleaved, records_ptr, cap, *head):
    """params: None (the library's defaults) or (min_overlap, max_mismatches, max_mismatch_pct).  Returns (InsertSummary, the
    histogram as a uint64 array of INSERT_HIST_BINS entries)."""
    import numpy as np
    hist = np.zeros(INSERT_HIST_BINS, dtype=np.uint64)
    s = _new_insert_summary()
    o = None
    if params is not None or interleaved:
        o = insert_opts(interleaved, *(params if params is not None else ()))
    rc = fn(*head, ctypes.byref(o) if o is not None else None, ctypes.c_void_p(records_ptr) if records_ptr else None, cap,
            ctypes.c_void_p(hist.ctypes.data), ctypes.byref(s))
    if rc != 0:
        e = ScfqError(rc, what, lib().scfq_insert_size_error_detail().decode() or lib().scfq_last_error_detail().decode())
        e.summary = s
        raise e
    return s, hist


def insert_size_device(ptr1, n1, ptr2=None, n2=0, params=None, records_ptr=None, cap=0):
    """fq-insert-size of device-resident FASTQs; ptr2 = None: ptr1 is interleaved.  records_ptr: device memory for `cap` OverlapRec
    entries (None: summary and histogram only; size it with the `pairs` of such a call)."""
    return _insert_call(lib().scfq_insert_size_buffers, "scfq_insert_size_buffers", params, ptr2 is None, records_ptr, cap,
                        ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1)


def insert_size_host(data1, data2=None, params=None, records_ptr=None, cap=0):
    """fq-insert-size of host buffers (bytes / numpy uint8); data2 = None: data1 is interleaved"""
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    return _insert_call(lib().scfq_insert_size_buffers, "scfq_insert_size_buffers", params, data2 is None, records_ptr, cap, a1, n1, a2, n2, 0)


def insert_size_file(path1, path2=None, params=None, records_ptr=None, cap=0):
    """path2 = None: path1 is interleaved"""
    return _insert_call(lib().scfq_insert_size_files, "scfq_insert_size_files", params, path2 is None, records_ptr, cap, os.fsencode(path1),
                        os.fsencode(path2) if path2 is not None else None, None)


def format_insert_size_tsv(s):
    buf = ctypes.create_string_buffer(1024)
    lib().scfq_format_insert_size_tsv(ctypes.byref(s), buf, 1024)
    return buf.value.decode()


def insert_size_stages():
    """(indexes, overlap kernel, pass over the bins, copy to the host) milliseconds of this thread's last insert_size call; the last
    three are HIP-event times and zeros unless SCFQ_INSERT_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_insert_size_stages(ms, 4)
    return list(ms)


def _new_merge_stats():
    s = MergeStats()
    s.struct_size = ctypes.sizeof(MergeStats)
    return s


def merge_opts(interleaved=False, min_overlap=30, max_mismatches=5, max_mismatch_pct=20, phred_offset=33):
    o = MergeOpts()
    o.struct_size = ctypes.sizeof(MergeOpts)
    o.flags = SCFQ_MERGE_INTERLEAVED if interleaved else 0
    o.min_overlap, o.max_mismatches, o.max_mismatch_pct, o.phred_offset = min_overlap, max_mismatches, max_mismatch_pct, phred_offset
    return o


def _merge_call(fn, what, params, phred_offset, interleaved, head, tail):
    """params: None (the library's defaults) or (min_overlap, max_mismatches, max_mismatch_pct).  Returns the MergeStats; an
    ScfqError carries them as `stats` (filled as far as the call got: complete when an output was too small)."""
    s = _new_merge_stats()
    o = None
    if params is not None or interleaved or phred_offset != 33:
        o = merge_opts(interleaved, *(params if params is not None else (30, 5, 20)), phred_offset)
    rc = fn(*head, ctypes.byref(o) if o is not None else None, *tail, ctypes.byref(s))
    if rc != 0:
        e = ScfqError(rc, what, lib().scfq_merge_error_detail().decode() or lib().scfq_last_error_detail().decode())
        e.stats = s
        raise e
    return s


def _merge_outputs(outs):
    """three (address, capacity) pairs or None -> the six arguments"""
    flat = []
    for o in outs:
        flat += [ctypes.c_void_p(o[0]) if o and o[0] else None, o[1] if o else 0]
    return flat


def merge_device(ptr1, n1, ptr2=None, n2=0, params=None, phred_offset=33, merged=None, un1=None, un2=None):
    """fq-merge of device-resident FASTQs; ptr2 = None: ptr1 is interleaved.  merged / un1 / un2: (device address, capacity) of an
    output, or None: not written, its size is in the stats all the same (three None: the sizing call)."""
    return _merge_call(lib().scfq_merge_buffers, "scfq_merge_buffers", params, phred_offset, ptr2 is None,
                       [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1], _merge_outputs((merged, un1, un2)) + [1])


def merge_host(data1, data2=None, params=None, phred_offset=33, caps=None):
    """fq-merge of host buffers (bytes / numpy uint8); data2 = None: data1 is interleaved.  caps: the capacities of the three outputs
    (an entry of None: that output is not produced); None: a sizing call first, then buffers that fit.  Returns (MergeStats,
    merged, unmerged1, unmerged2), the outputs as bytes or None."""
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    head = [a1, n1, a2, n2, 0]
    fn = lib().scfq_merge_buffers
    if caps is None:
        s = _merge_call(fn, "scfq_merge_buffers", params, phred_offset, data2 is None, head, [None, 0, None, 0, None, 0, 0])
        caps = (s.merged_bytes, s.unmerged1_bytes, s.unmerged2_bytes if data2 is not None else None)
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s = _merge_call(fn, "scfq_merge_buffers", params, phred_offset, data2 is None, head, _merge_outputs(outs) + [0])
    sizes = (s.merged_bytes, s.unmerged1_bytes, s.unmerged2_bytes)
    return (s,) + tuple(None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes))


def merge_file(path1, path2=None, params=None, phred_offset=33, merged_fd=-1, un1_fd=-1, un2_fd=-1):
    """path2 = None: path1 is interleaved.  A descriptor below 0: that output is not produced.  The outputs are written one after
    another, each in full."""
    return _merge_call(lib().scfq_merge_files, "scfq_merge_files", params, phred_offset, path2 is None,
                       [os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, None], [merged_fd, un1_fd, un2_fd])


def format_merge_stats_tsv(s):
    buf = ctypes.create_string_buffer(1024)
    lib().scfq_format_merge_stats_tsv(ctypes.byref(s), buf, 1024)
    return buf.value.decode()


def merge_stages():
    """(indexes, overlap kernel, lengths and scans, write kernel) milliseconds of this thread's last merge call; the last three are
    HIP-event times and zeros unless SCFQ_MERGE_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_merge_stages(ms, 4)
    return list(ms)


def _new_trim_stats():
    s = TrimStats()
    s.struct_size = ctypes.sizeof(TrimStats)
    return s


def trim_opts(interleaved=False, no_overlap=False, no_adapters=False, probes=None, min_overlap=30, max_mismatches=5, max_mismatch_pct=20,
              min_adapter_overlap=5, adapter_mismatch_pct=10, poly_g=0, window=4, window_quality=0, min_length=15, phred_offset=33):
    """probes: None (the built-in set, or none with no_adapters) or up to eight sequences (bytes or str)"""
    o = TrimOpts()
    o.struct_size = ctypes.sizeof(TrimOpts)
    o.flags = (SCFQ_TRIM_INTERLEAVED if interleaved else 0) | (SCFQ_TRIM_NO_OVERLAP if no_overlap else 0) | (SCFQ_TRIM_NO_ADAPTERS if no_adapters else 0)
    o.min_overlap, o.max_mismatches, o.max_mismatch_pct = min_overlap, max_mismatches, max_mismatch_pct
    o.min_adapter_overlap, o.adapter_mismatch_pct, o.poly_g = min_adapter_overlap, adapter_mismatch_pct, poly_g
    o.window, o.window_quality, o.min_length, o.phred_offset = window, window_quality, min_length, phred_offset
    seqs = [p.encode() if isinstance(p, str) else bytes(p) for p in (probes or ())]
    o.n_probes = len(seqs)
    for j, p in enumerate(seqs[:8]):
        o.probes[j] = p
    return o


def _trim_call(fn, what, opts, head, tail):
    """opts: None (the library's defaults) or a TrimOpts.  Returns the TrimStats; an ScfqError carries them as `stats` (filled as far
    as the call got: complete when an output was too small)."""
    s = _new_trim_stats()
    rc = fn(*head, ctypes.byref(opts) if opts is not None else None, *tail, ctypes.byref(s))
    if rc != 0:
        e = ScfqError(rc, what, lib().scfq_trim_error_detail().decode() or lib().scfq_last_error_detail().decode())
        e.stats = s
        raise e
    return s


def _trim_outputs(outs):
    """two (address, capacity) pairs or None -> the four arguments"""
    flat = []
    for o in outs:
        flat += [ctypes.c_void_p(o[0]) if o and o[0] else None, o[1] if o else 0]
    return flat


def trim_device(ptr1, n1, ptr2=None, n2=0, opts=None, out1=None, out2=None):
    """fq-trim of device-resident FASTQs; ptr2 = None: ptr1 is single-end or, with the flag in opts, interleaved.  out1 / out2: (device
    address, capacity) of an output, or None: not written, its size is in the stats all the same (two None: the sizing call)."""
    return _trim_call(lib().scfq_trim_buffers, "scfq_trim_buffers", opts,
                      [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1], _trim_outputs((out1, out2)) + [1])


def trim_host(data1, data2=None, opts=None, caps=None):
    """fq-trim of host buffers (bytes / numpy uint8); data2 = None: one input.  caps: the capacities of the two outputs (an entry of
    None: that output is not produced); None: a sizing call first, then buffers that fit.  Returns (TrimStats, out1, out2), the outputs
    as bytes or None."""
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    head = [a1, n1, a2, n2, 0]
    fn = lib().scfq_trim_buffers
    if caps is None:
        s = _trim_call(fn, "scfq_trim_buffers", opts, head, [None, 0, None, 0, 0])
        caps = (s.out1_bytes, s.out2_bytes if data2 is not None else None)
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s = _trim_call(fn, "scfq_trim_buffers", opts, head, _trim_outputs(outs) + [0])
    sizes = (s.out1_bytes, s.out2_bytes)
    return (s,) + tuple(None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes))


def trim_file(path1, path2=None, opts=None, out1_fd=-1, out2_fd=-1):
    """path2 = None: one input.  A descriptor below 0: that output is not produced.  The outputs are written one after the other."""
    return _trim_call(lib().scfq_trim_files, "scfq_trim_files", opts,
                      [os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, None], [out1_fd, out2_fd])


def format_trim_stats_tsv(s):
    buf = ctypes.create_string_buffer(1024)
    lib().scfq_format_trim_stats_tsv(ctypes.byref(s), buf, 1024)
    return buf.value.decode()


def trim_stages():
    """(overlap kernel, decision kernel, lengths and scans, write kernel) milliseconds of this thread's last trim call: HIP-event times,
    zeros unless SCFQ_TRIM_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_trim_stages(ms, 4)
    return list(ms)


def _screen_error(rc, what):
    return ScfqError(rc, what, lib().scfq_screen_error_detail().decode() or lib().scfq_last_error_detail().decode())


class ScreenIndex:
    """scfq_screen_index: the k-mer table of up to 16 references on the device.  `summary` is the ScreenSummary of the build, `names` the
    references' names.  close() (or the end of a `with`) frees it."""

    def __init__(self, handle, summary):
        self._h, self.summary = handle, summary
        self.names = [lib().scfq_screen_ref_name(handle, r).decode("latin-1") for r in range(summary.n_refs)]
        self.k = int(summary.k)

    @property
    def handle(self):
        return self._h

    def build_ms(self):
        return lib().scfq_debug_screen_build_ms(self._h)

    def close(self):
        if self._h:
            lib().scfq_screen_index_free(self._h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _new_screen_summary():
    s = ScreenSummary()
    s.struct_size = ctypes.sizeof(ScreenSummary)
    return s


def screen_index_host(refs, k=31):
    """refs: a list of (name, FASTA text as bytes / numpy uint8)"""
    arr = (ScreenRef * max(len(refs), 1))()
    keep = []
    for i, (name, text) in enumerate(refs[:len(arr)]):
        addr, n, held = _host_ptr(text)
        raw = name.encode("latin-1") if isinstance(name, str) else name
        keep.append((held, raw))
        arr[i] = ScreenRef(raw, addr.value if hasattr(addr, "value") else addr, n)
    h, s = ctypes.c_void_p(), _new_screen_summary()
    rc = lib().scfq_screen_index_buffers(arr, len(refs), k, ctypes.byref(h), ctypes.byref(s))
    if rc != 0:
        raise _screen_error(rc, "scfq_screen_index_buffers")
    return ScreenIndex(h, s)


def screen_index_files(paths, names=None, k=31):
    """names: None, or a list with a name or None (the file's base name up to its first '.') per path"""
    n = len(paths)
    pa = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
    na = None
    if names is not None:
        na = (ctypes.c_char_p * max(n, 1))(*[None if x is None else (x.encode("latin-1") if isinstance(x, str) else x) for x in names])
    h, s = ctypes.c_void_p(), _new_screen_summary()
    rc = lib().scfq_screen_index_files(na, pa, n, k, None, ctypes.byref(h), ctypes.byref(s))
    if rc != 0:
        raise _screen_error(rc, "scfq_screen_index_files")
    return ScreenIndex(h, s)


def screen_opts(interleaved=False, keep_matched=False, min_hits=1, min_hit_pct=0, flags=None, reserved=0):
    o = ScreenOpts()
    o.struct_size = ctypes.sizeof(ScreenOpts)
    o.flags = flags if flags is not None else (SCFQ_SCREEN_INTERLEAVED if interleaved else 0) | (SCFQ_SCREEN_KEEP_MATCHED if keep_matched else 0)
    o.min_hits, o.min_hit_pct, o.reserved = min_hits, min_hit_pct, reserved
    return o


def _screen_call(fn, what, index, opts, head, tail):
    """Returns the ScreenStats; an ScfqError carries them as `stats` (complete when an output was too small)."""
    s = ScreenStats()
    s.struct_size = ctypes.sizeof(ScreenStats)
    handle = index.handle if isinstance(index, ScreenIndex) else index
    rc = fn(handle, *head, ctypes.byref(opts) if opts is not None else None, *tail, ctypes.byref(s))
    if rc != 0:
        e = _screen_error(rc, what)
        e.stats = s
        raise e
    return s


def screen_device(index, ptr1, n1, ptr2=None, n2=0, opts=None, out1=None, out2=None, recs=None):
    """fq-screen of device-resident FASTQs (the pointer rules of trim_device).  out1 / out2: (device address, capacity) or None; recs:
    (device address, entries) of the per-read table or None."""
    return _screen_call(lib().scfq_screen_buffers, "scfq_screen_buffers", index, opts,
                        [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1],
                        [ctypes.c_void_p(recs[0]) if recs else None, recs[1] if recs else 0] + _trim_outputs((out1, out2)) + [1])


def screen_host(index, data1, data2=None, opts=None, caps=None):
    """fq-screen of host buffers; caps as trim_host's.  Returns (ScreenStats, out1, out2), the outputs as bytes or None."""
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    head = [a1, n1, a2, n2, 0]
    fn = lib().scfq_screen_buffers
    if caps is None:
        s = _screen_call(fn, "scfq_screen_buffers", index, opts, head, [None, 0, None, 0, None, 0, 0])
        caps = (s.out1_bytes, s.out2_bytes if data2 is not None else None)
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s = _screen_call(fn, "scfq_screen_buffers", index, opts, head, [None, 0] + _trim_outputs(outs) + [0])
    sizes = (s.out1_bytes, s.out2_bytes)
    return (s,) + tuple(None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes))


def screen_file(index, path1, path2=None, opts=None, out1_fd=-1, out2_fd=-1, recs=None):
    """recs: None, or a ctypes array of ScreenRec that receives the per-read table"""
    return _screen_call(lib().scfq_screen_files, "scfq_screen_files", index, opts,
                        [os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, None],
                        [out1_fd, out2_fd, ctypes.cast(recs, ctypes.c_void_p) if recs is not None else None, len(recs) if recs is not None else 0])


def format_screen_row_tsv(s, index, r):
    buf = ctypes.create_string_buffer(1024)
    n = lib().scfq_format_screen_row_tsv(ctypes.byref(s), index.handle, r, buf, 1024)
    if n < 0:
        raise ScfqError(n, "scfq_format_screen_row_tsv")
    return buf.value.decode("latin-1")


def screen_stages():
    """(line indexes of paired input, lookup kernel, lengths and scans, write kernel) milliseconds of this thread's last screen call; the
    last three are HIP-event times and zeros unless SCFQ_SCREEN_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_screen_stages(ms, 4)
    return list(ms)


def _demux_error(rc, what):
    return ScfqError(rc, what, lib().scfq_demux_error_detail().decode() or lib().scfq_last_error_detail().decode())


class DemuxSheet:
    """scfq_demux_sheet: the samples of a run, host memory only.  `names` has N + 1 entries, the last one "undetermined"; `samples` the
    (name, barcode1, barcode2 or None) triples as given.  close() (or the end of a `with`) frees it."""

    def __init__(self, handle, samples):
        self._h, self.samples = handle, samples
        self.n = int(lib().scfq_demux_sheet_samples(handle))
        self.names = [lib().scfq_demux_sheet_name(handle, s).decode("latin-1") for s in range(self.n + 1)]

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().scfq_demux_sheet_free(self._h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def demux_sheet(samples):
    """samples: a list of (name, barcode1) or (name, barcode1, barcode2), each bytes or str (None stays NULL)"""
    raw = lambda x: None if x is None else (x.encode("latin-1") if isinstance(x, str) else bytes(x))
    triples = [(raw(t[0]), raw(t[1]), raw(t[2]) if len(t) > 2 else None) for t in samples]
    arr = (DemuxSample * max(len(triples), 1))()
    for i, t in enumerate(triples):
        arr[i] = DemuxSample(*t)
    h = ctypes.c_void_p()
    rc = lib().scfq_demux_sheet_new(arr, len(triples), ctypes.byref(h))
    if rc != 0:
        raise _demux_error(rc, "scfq_demux_sheet_new")
    return DemuxSheet(h, triples)


def demux_opts(interleaved=False, header=False, keep_barcode=False, mismatches=1, flags=None, reserved=(0, 0)):
    o = DemuxOpts()
    o.struct_size = ctypes.sizeof(DemuxOpts)
    o.flags = flags if flags is not None else (SCFQ_DEMUX_INTERLEAVED if interleaved else 0) | (SCFQ_DEMUX_HEADER if header else 0) | \
        (SCFQ_DEMUX_KEEP_BARCODE if keep_barcode else 0)
    o.mismatches = mismatches
    o.reserved[0], o.reserved[1] = reserved
    return o


def _demux_call(fn, what, sheet, opts, head, mid, tail, row_cap=None):
    """Returns (DemuxStats, rows): rows is a list of N + 1 DemuxRow.  An ScfqError carries both as `stats` and `rows` (complete when an
    output was too small).  row_cap: the capacity told to the library, None: N + 1."""
    s = DemuxStats()
    s.struct_size = ctypes.sizeof(DemuxStats)
    n = sheet.n if isinstance(sheet, DemuxSheet) else 0
    rows = (DemuxRow * (n + 1))()
    handle = sheet.handle if isinstance(sheet, DemuxSheet) else sheet
    rc = fn(handle, *head, ctypes.byref(opts) if opts is not None else None, *mid, ctypes.cast(rows, ctypes.c_void_p), n + 1 if row_cap is None else row_cap,
            *tail, ctypes.byref(s))
    if rc != 0:
        e = _demux_error(rc, what)
        e.stats, e.rows = s, list(rows)
        raise e
    return s, list(rows)


def demux_device(sheet, ptr1, n1, ptr2=None, n2=0, opts=None, out1=None, out2=None, recs=None, row_cap=None):
    """fq-demux of device-resident FASTQs (the pointer rules of trim_device).  out1 / out2: (device address, capacity) or None; recs:
    (device address, entries) of the per-unit table or None.  Returns (DemuxStats, rows)."""
    return _demux_call(lib().scfq_demux_buffers, "scfq_demux_buffers", sheet, opts,
                       [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1],
                       [ctypes.c_void_p(recs[0]) if recs else None, recs[1] if recs else 0], _trim_outputs((out1, out2)) + [1], row_cap)


def demux_host(sheet, data1, data2=None, opts=None, caps=None):
    """fq-demux of host buffers; caps as trim_host's.  Returns (DemuxStats, rows, out1, out2), the outputs as bytes or None."""
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    head = [a1, n1, a2, n2, 0]
    fn = lib().scfq_demux_buffers
    if caps is None:
        s, rows = _demux_call(fn, "scfq_demux_buffers", sheet, opts, head, [None, 0], [None, 0, None, 0, 0])
        caps = (s.out1_bytes, s.out2_bytes if data2 is not None else None)
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s, rows = _demux_call(fn, "scfq_demux_buffers", sheet, opts, head, [None, 0], _trim_outputs(outs) + [0])
    sizes = (s.out1_bytes, s.out2_bytes)
    return (s, rows) + tuple(None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes))


def demux_file(sheet, path1, path2=None, opts=None, out_dir=None, recs=None):
    """out_dir: None (report only) or an existing directory that receives a file per destination and mate.  recs: None, or a ctypes
    array of DemuxRec that receives the per-unit table.  Returns (DemuxStats, rows)."""
    return _demux_call(lib().scfq_demux_files, "scfq_demux_files", sheet, opts,
                       [os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, None],
                       [os.fsencode(out_dir) if out_dir is not None else None, ctypes.cast(recs, ctypes.c_void_p) if recs is not None else None,
                        len(recs) if recs is not None else 0], [])


def format_demux_row_tsv(s, sheet, d, row):
    buf = ctypes.create_string_buffer(1024)
    n = lib().scfq_format_demux_row_tsv(ctypes.byref(s), sheet.handle, d, ctypes.byref(row), buf, 1024)
    if n < 0:
        raise ScfqError(n, "scfq_format_demux_row_tsv")
    return buf.value.decode("latin-1")


def demux_stages():
    """(assignment kernel, radix sort, lengths and scans, gather-write kernel) milliseconds of this thread's last demux call: HIP-event
    times, zeros unless SCFQ_DEMUX_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_demux_stages(ms, 4)
    return list(ms)


def _kcount_error(rc, what):
    return ScfqError(rc, what, lib().scfq_kcount_error_detail().decode() or lib().scfq_last_error_detail().decode())


class KcountTable:
    """scfq_kcount: the table of one fq-kcount call, on the device.  close() (or the end of a `with`) frees it."""

    def __init__(self, handle, k, flags):
        self._h, self.k, self.flags = handle, k, flags

    @property
    def handle(self):
        return self._h

    def hist(self, bins):
        """numpy uint64 array of `bins` entries: [c] keys with count c, the last one keys with count >= bins - 1"""
        import numpy as np
        out = np.zeros(max(int(bins), 1), dtype=np.uint64)
        rc = lib().scfq_kcount_hist(self._h, out.ctypes.data, bins)
        if rc != 0:
            raise _kcount_error(rc, "scfq_kcount_hist")
        return out

    def dump_into(self, out, cap, min_count=1, max_count=0):
        """the raw call: out is a numpy uint64 array of shape (rows, 2) or None; returns total"""
        total = ctypes.c_uint64(0)
        rc = lib().scfq_kcount_dump(self._h, min_count, max_count, out.ctypes.data if out is not None else None, cap, ctypes.byref(total))
        if rc != 0:
            raise _kcount_error(rc, "scfq_kcount_dump")
        return int(total.value)

    def dump(self, min_count=1, max_count=0):
        """numpy uint64 array of shape (total, 2): (key, count) in ascending key order"""
        import numpy as np
        total = self.dump_into(None, 0, min_count, max_count)
        out = np.zeros((total, 2), dtype=np.uint64)
        if total:
            assert self.dump_into(out, total, min_count, max_count) == total
        return out

    def query(self, keys):
        """numpy uint64 array: the count of every key (plain indices), 0 when absent"""
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(keys.size, dtype=np.uint64)
        rc = lib().scfq_kcount_query(self._h, keys.ctypes.data if keys.size else None, keys.size, out.ctypes.data if keys.size else None)
        if rc != 0:
            raise _kcount_error(rc, "scfq_kcount_query")
        return out

    def close(self):
        if self._h:
            lib().scfq_kcount_free(self._h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def kcount_opts(k=21, flags=0, table_bits=0, reserved=0):
    o = KcountOpts()
    o.struct_size = ctypes.sizeof(KcountOpts)
    o.k, o.flags, o.table_bits, o.reserved = k, flags, table_bits, reserved
    return o


def _new_kcount_summary():
    s = KcountSummary()
    s.struct_size = ctypes.sizeof(KcountSummary)
    return s


def _kcount_call(fn, what, head, k, flags, table_bits, table):
    """Returns (KcountSummary, KcountTable), the table None with table=False"""
    s = _new_kcount_summary()
    o = kcount_opts(k, flags, table_bits)
    h = ctypes.c_void_p()
    rc = fn(*head, ctypes.byref(o), ctypes.byref(h) if table else None, ctypes.byref(s))
    if rc != 0:
        e = _kcount_error(rc, what)
        e.handle = h.value
        raise e
    return s, (KcountTable(h, k, flags) if table else None)


def kcount_device(ptr1, n1, ptr2=None, n2=0, k=21, flags=0, table_bits=0, table=True):
    """fq-kcount of one or two device-resident FASTQs (counted into one table)"""
    return _kcount_call(lib().scfq_kcount_buffers, "scfq_kcount_buffers",
                        [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1], k, flags, table_bits, table)


def kcount_host(data1, data2=None, k=21, flags=0, table_bits=0, table=True):
    """fq-kcount of one or two host buffers (bytes / numpy uint8)"""
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    return _kcount_call(lib().scfq_kcount_buffers, "scfq_kcount_buffers", [a1, n1, a2, n2, 0], k, flags, table_bits, table)


def kcount_files(path1, path2=None, k=21, flags=0, table_bits=0, table=True):
    return _kcount_call(lib().scfq_kcount_files, "scfq_kcount_files",
                        [os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, None], k, flags, table_bits, table)


def format_kcount_tsv(k, key, count):
    buf = ctypes.create_string_buffer(96)
    n = lib().scfq_format_kcount_tsv(k, key, count, buf, 96)
    if n < 0:
        raise ScfqError(n, "scfq_format_kcount_tsv")
    return buf.value.decode()


def kcount_stages():
    """(line indexes, H1 of the last pass, H2, H3 of the last hist) milliseconds of this thread's last kcount calls; the last three
    are HIP-event times, zeros unless SCFQ_KCOUNT_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_kcount_stages(ms, 4)
    return list(ms)


def _norm_error(rc, what):
    return ScfqError(rc, what, lib().scfq_norm_error_detail().decode() or lib().scfq_last_error_detail().decode())


def norm_opts(interleaved=False, keep_no_kmers=False, k=0, canonical=False, table_bits=0, target=0, min_depth=0, weak_below=2, seed=0,
              flags=None, table_flags=None, reserved=0):
    """scfq_norm_opts.  k, canonical and table_bits matter without a table only (the two-pass form)"""
    o = NormOpts()
    o.struct_size = ctypes.sizeof(NormOpts)
    o.flags = flags if flags is not None else (SCFQ_NORM_INTERLEAVED if interleaved else 0) | (SCFQ_NORM_KEEP_NO_KMERS if keep_no_kmers else 0)
    o.table_flags = table_flags if table_flags is not None else (SCFQ_KCOUNT_CANONICAL if canonical else 0)
    o.k, o.table_bits, o.target, o.min_depth, o.weak_below, o.reserved, o.seed = k, table_bits, target, min_depth, weak_below, reserved, seed
    return o


def _norm_call(fn, what, table, opts, head, tail, bins):
    """Returns (NormStats, hist): hist a numpy uint64 array of shape (bins, 2) with the columns (units in, units kept), or None with
    bins = 0.  An ScfqError carries the stats as `stats` (complete when an output was too small)."""
    import numpy as np
    s = NormStats()
    s.struct_size = ctypes.sizeof(NormStats)
    hist = np.zeros((bins, 2), dtype=np.uint64) if bins else None
    handle = table.handle if isinstance(table, KcountTable) else table
    rc = fn(handle, *head, ctypes.byref(opts) if opts is not None else None, *tail, hist.ctypes.data if bins else None, bins, ctypes.byref(s))
    if rc != 0:
        e = _norm_error(rc, what)
        e.stats = s
        raise e
    return s, hist


def norm_device(table, ptr1, n1, ptr2=None, n2=0, opts=None, out1=None, out2=None, recs=None, bins=0):
    """fq-normalize of device-resident FASTQs against a KcountTable (None: the two-pass form; the pointer rules of trim_device).
    out1 / out2: (device address, capacity) or None; recs: (device address, entries) of the per-read table or None."""
    return _norm_call(lib().scfq_norm_buffers, "scfq_norm_buffers", table, opts,
                      [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1],
                      [ctypes.c_void_p(recs[0]) if recs else None, recs[1] if recs else 0] + _trim_outputs((out1, out2)) + [1], bins)


def norm_host(table, data1, data2=None, opts=None, caps=None, bins=0):
    """fq-normalize of host buffers; caps as trim_host's.  Returns (NormStats, hist, out1, out2), the outputs as bytes or None."""
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    head = [a1, n1, a2, n2, 0]
    fn = lib().scfq_norm_buffers
    if caps is None:
        s, _ = _norm_call(fn, "scfq_norm_buffers", table, opts, head, [None, 0, None, 0, None, 0, 0], 0)
        caps = (s.out1_bytes, s.out2_bytes if data2 is not None else None)
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s, hist = _norm_call(fn, "scfq_norm_buffers", table, opts, head, [None, 0] + _trim_outputs(outs) + [0], bins)
    sizes = (s.out1_bytes, s.out2_bytes)
    return (s, hist) + tuple(None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes))


def norm_file(table, path1, path2=None, opts=None, out1_fd=-1, out2_fd=-1, recs=None, bins=0):
    """recs: None, or a ctypes array of NormRec that receives the per-read table.  Returns (NormStats, hist)"""
    return _norm_call(lib().scfq_norm_files, "scfq_norm_files", table, opts,
                      [os.fsencode(path1) if path1 is not None else None, os.fsencode(path2) if path2 is not None else None, None],
                      [out1_fd, out2_fd, ctypes.cast(recs, ctypes.c_void_p) if recs is not None else None, len(recs) if recs is not None else 0], bins)


def format_norm_row_tsv(s, header=False):
    buf = ctypes.create_string_buffer(1024)
    n = lib().scfq_format_norm_row_tsv(ctypes.byref(s) if s is not None else None, 1 if header else 0, buf, 1024)
    if n < 0:
        raise ScfqError(n, "scfq_format_norm_row_tsv")
    return buf.value.decode()


def format_norm_hist_tsv(depth, units_in, units_out):
    buf = ctypes.create_string_buffer(96)
    lib().scfq_format_norm_hist_tsv(depth, units_in, units_out, buf, 96)
    return buf.value.decode()


def norm_stages():
    """(line indexes, N1, N2 with its scans, N3) milliseconds of this thread's last normalize call; the last three are HIP-event times,
    zeros unless SCFQ_NORM_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_norm_stages(ms, 4)
    return list(ms)


def cplx_opts(interleaved=False, window=64, threshold=20, mask="lower", max_masked_pct=100, flags=None, reserved=(0, 0, 0)):
    """scfq_cplx_opts.  mask: "none", "lower", "n" or the number"""
    o = CplxOpts()
    o.struct_size = ctypes.sizeof(CplxOpts)
    o.flags = flags if flags is not None else (SCFQ_CPLX_INTERLEAVED if interleaved else 0)
    o.window, o.threshold, o.mask, o.max_masked_pct = window, threshold, CPLX_MASKS.get(mask, mask), max_masked_pct
    for k in range(3):
        o.reserved[k] = reserved[k]
    return o


def _cplx_call(fn, what, opts, head, tail, hist=True):
    """Returns (CplxStats, hist): hist a numpy uint64 array of SCFQ_CPLX_SCORE_BINS entries, or None.  An ScfqError carries the stats as
    `stats` (complete when an output or the per-read table was too small)."""
    import numpy as np
    s = CplxStats()
    s.struct_size = ctypes.sizeof(CplxStats)
    h = np.zeros(SCFQ_CPLX_SCORE_BINS, dtype=np.uint64) if hist else None
    rc = fn(*head, ctypes.byref(opts) if opts is not None else None, *tail(h.ctypes.data if hist else None), ctypes.byref(s))
    if rc != 0:
        e = ScfqError(rc, what, lib().scfq_cplx_error_detail().decode() or lib().scfq_last_error_detail().decode())
        e.stats = s
        raise e
    return s, h


def cplx_resident(ptr1, n1, ptr2=None, n2=0, opts=None, out1=None, out2=None, recs=None, hist=True):
    """fq-complexity of device-resident FASTQs (the pointer rules of trim_device; not named *_device: tests/_caller_cases.py lists the wrappers
    of that name, and this one's caller-stream and thread tests are tests/test_gpu_complexity_callers.py's).  out1 / out2: (device address, capacity) or None; recs:
    (device address, entries) of the per-read table or None.  Returns (CplxStats, hist)."""
    return _cplx_call(lib().scfq_cplx_buffers, "scfq_cplx_buffers", opts,
                      [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1],
                      lambda h: [ctypes.c_void_p(recs[0]) if recs else None, recs[1] if recs else 0, h] + _trim_outputs((out1, out2)) + [1], hist)


def cplx_host(data1, data2=None, opts=None, caps=None, recs_cap=None, hist=True):
    """fq-complexity of host buffers; caps as trim_host's; recs_cap: the entries of the per-read table (None: as many as there are reads,
    0: no table).  Returns (CplxStats, hist, recs, out1, out2): recs a numpy array of CPLX_REC_DTYPE or None, the outputs as bytes or None."""
    import numpy as np
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    head = [a1, n1, a2, n2, 0]
    fn = lib().scfq_cplx_buffers
    if caps is None or recs_cap is None:
        s, _ = _cplx_call(fn, "scfq_cplx_buffers", opts, head, lambda h: [None, 0, h, None, 0, None, 0, 0], False)
        if caps is None:
            caps = (s.out1_bytes, s.out2_bytes if data2 is not None else None)
        if recs_cap is None:
            recs_cap = int(s.reads_in)
    recs = np.zeros(recs_cap, dtype=np.dtype(CPLX_REC_DTYPE)) if recs_cap else None
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s, h = _cplx_call(fn, "scfq_cplx_buffers", opts, head,
                      lambda h: [recs.ctypes.data if recs_cap else None, recs_cap, h] + _trim_outputs(outs) + [0], hist)
    sizes = (s.out1_bytes, s.out2_bytes)
    return (s, h, recs[:int(s.reads_in)] if recs_cap else None) + tuple(None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes))


def cplx_files(path1, path2=None, opts=None, out1_fd=-1, out2_fd=-1, per_read_fd=-1, hist=True):
    """path2 = None: one input.  A descriptor below 0: that output is not produced.  Returns (CplxStats, hist)"""
    return _cplx_call(lib().scfq_cplx_files, "scfq_cplx_files", opts, [os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, None],
                      lambda h: [out1_fd, out2_fd, per_read_fd, h], hist)


def format_cplx_stats_tsv(s, header=False):
    buf = ctypes.create_string_buffer(1024)
    n = lib().scfq_format_cplx_stats_tsv(ctypes.byref(s) if s is not None else None, 1 if header else 0, buf, 1024)
    if n < 0:
        raise ScfqError(n, "scfq_format_cplx_stats_tsv")
    return buf.value.decode()


def format_cplx_rec_tsv(read, rec, length):
    """rec: None (the column names), a CplxRec or a (score, masked, first, intervals) tuple"""
    buf = ctypes.create_string_buffer(160)
    r = rec if rec is None or isinstance(rec, CplxRec) else CplxRec(*[int(v) for v in rec])
    lib().scfq_format_cplx_rec_tsv(read, ctypes.byref(r) if r is not None else None, length, buf, 160)
    return buf.value.decode()


def cplx_stages():
    """(line indexes, D1, D2 with its scans, D3) milliseconds of this thread's last fq-complexity call; the last three are HIP-event times,
    zeros unless SCFQ_CPLX_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_cplx_stages(ms, 4)
    return list(ms)


def rmdup_opts(interleaved=False, swapped=False, prefix=0, hash_bits=0, flags=None, reserved=(0, 0, 0)):
    """scfq_rmdup_opts.  prefix: 0 (the whole sequence text) or the bytes of it that are compared; hash_bits: 0 (the library's default) or the
    bits of the hash that are sorted"""
    o = RmdupOpts()
    o.struct_size = ctypes.sizeof(RmdupOpts)
    o.flags = flags if flags is not None else ((SCFQ_RMDUP_INTERLEAVED if interleaved else 0) | (SCFQ_RMDUP_SWAPPED if swapped else 0))
    o.prefix, o.hash_bits = prefix, hash_bits
    for k in range(3):
        o.reserved[k] = reserved[k]
    return o


def _rmdup_call(fn, what, head, tail, hist=True):
    """Returns (RmdupStats, hist): hist a numpy uint64 array of SCFQ_RMDUP_HIST_BINS entries, or None.  An ScfqError carries the stats as
    `stats` (complete when an output or the per-unit table was too small)."""
    import numpy as np
    s = RmdupStats()
    s.struct_size = ctypes.sizeof(RmdupStats)
    h = np.zeros(SCFQ_RMDUP_HIST_BINS, dtype=np.uint64) if hist else None
    rc = fn(*head, *tail(h.ctypes.data if hist else None), ctypes.byref(s))
    if rc != 0:
        e = ScfqError(rc, what, lib().scfq_rmdup_error_detail().decode() or lib().scfq_last_error_detail().decode())
        e.stats = s
        raise e
    return s, h


def _opts_ref(opts):
    return ctypes.byref(opts) if opts is not None else None


def rmdup_resident(ptr1, n1, ptr2=None, n2=0, opts=None, out1=None, out2=None, recs=None, hist=True):
    """fq-rmdup of device-resident FASTQs (the pointer rules of trim_device; not named *_device: tests/_caller_cases.py lists the wrappers
    of that name, and this one's caller-stream and thread tests are tests/test_gpu_rmdup_callers.py's).  out1 / out2: (device address,
    capacity) or None; recs: (device address, entries) of the per-unit table or None.  Returns (RmdupStats, hist)."""
    return _rmdup_call(lib().scfq_rmdup_buffers, "scfq_rmdup_buffers",
                       [ctypes.c_void_p(ptr1), n1, ctypes.c_void_p(ptr2) if ptr2 is not None else None, n2, 1, _opts_ref(opts)],
                       lambda h: [ctypes.c_void_p(recs[0]) if recs else None, recs[1] if recs else 0, h] + _trim_outputs((out1, out2)) + [1], hist)


def rmdup_host(data1, data2=None, opts=None, caps=None, recs_cap=None, hist=True):
    """fq-rmdup of host buffers; caps as trim_host's; recs_cap: the entries of the per-unit table (None: as many as there are units,
    0: no table).  Returns (RmdupStats, hist, recs, out1, out2): recs a numpy array of RMDUP_REC_DTYPE or None, the outputs as bytes or None."""
    import numpy as np
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2) if data2 is not None else (None, 0, None)
    head = [a1, n1, a2, n2, 0, _opts_ref(opts)]
    fn = lib().scfq_rmdup_buffers
    if caps is None or recs_cap is None:
        s, _ = _rmdup_call(fn, "scfq_rmdup_buffers", head, lambda h: [None, 0, h, None, 0, None, 0, 0], False)
        if caps is None:
            caps = (s.out1_bytes, s.out2_bytes if data2 is not None else None)
        if recs_cap is None:
            recs_cap = int(s.units_in)
    recs = np.zeros(recs_cap, dtype=np.dtype(RMDUP_REC_DTYPE)) if recs_cap else None
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s, h = _rmdup_call(fn, "scfq_rmdup_buffers", head,
                       lambda h: [recs.ctypes.data if recs_cap else None, recs_cap, h] + _trim_outputs(outs) + [0], hist)
    sizes = (s.out1_bytes, s.out2_bytes)
    return (s, h, recs[:int(s.units_in)] if recs_cap else None) + tuple(None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes))


def rmdup_files(path1, path2=None, opts=None, out1_fd=-1, out2_fd=-1, per_read_fd=-1, hist=True):
    """path2 = None: one input.  A descriptor below 0: that output is not produced.  Returns (RmdupStats, hist)"""
    return _rmdup_call(lib().scfq_rmdup_files, "scfq_rmdup_files",
                       [os.fsencode(path1), os.fsencode(path2) if path2 is not None else None, _opts_ref(opts), None],
                       lambda h: [out1_fd, out2_fd, per_read_fd, h], hist)


def format_rmdup_stats_tsv(s, header=False):
    buf = ctypes.create_string_buffer(1024)
    n = lib().scfq_format_rmdup_stats_tsv(ctypes.byref(s) if s is not None else None, 1 if header else 0, buf, 1024)
    if n < 0:
        raise ScfqError(n, "scfq_format_rmdup_stats_tsv")
    return buf.value.decode()


def format_rmdup_rec_tsv(unit, rec):
    """rec: None (the column names), an RmdupRec or a (rep, copies) tuple"""
    buf = ctypes.create_string_buffer(96)
    r = rec if rec is None or isinstance(rec, RmdupRec) else RmdupRec(*[int(v) for v in rec])
    lib().scfq_format_rmdup_rec_tsv(unit, ctypes.byref(r) if r is not None else None, buf, 96)
    return buf.value.decode()


def rmdup_stages():
    """(line indexes, U1, sort, U2 + U3 rounds, class sizes, U4 with its scans, U5) milliseconds of this thread's last fq-rmdup call; all but
    the first are HIP-event times, zeros unless SCFQ_RMDUP_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 7)()
    lib().scfq_debug_rmdup_stages(ms, 7)
    return list(ms)


def repair_opts(hash_bits=0, flags=0, reserved=(0, 0, 0, 0)):
    """scfq_repair_opts.  hash_bits: 0 (the library's default) or the bits of the name hash that are sorted; every flag bit is reserved"""
    o = RepairOpts()
    o.struct_size = ctypes.sizeof(RepairOpts)
    o.flags, o.hash_bits = flags, hash_bits
    for k in range(4):
        o.reserved[k] = reserved[k]
    return o


def _repair_call(fn, what, args):
    """Returns RepairStats.  An ScfqError carries the stats as `stats` (complete when an output or the table was too small)."""
    s = RepairStats()
    s.struct_size = ctypes.sizeof(RepairStats)
    rc = fn(*args, ctypes.byref(s))
    if rc != 0:
        e = ScfqError(rc, what, lib().scfq_repair_error_detail().decode() or lib().scfq_last_error_detail().decode())
        e.stats = s
        raise e
    return s


def _repair_outputs(outs):
    """four (address, capacity) pairs or None -> the eight arguments"""
    outs = tuple(outs or ()) + (None,) * (4 - len(outs or ()))
    return _trim_outputs(outs)


def repair_resident(ptr1, n1, ptr2, n2, opts=None, outs=None, table=None):
    """fq-repair of two device-resident FASTQs (the pointer rules of trim_device; not named *_device: tests/_caller_cases.py lists the
    wrappers of that name, and this one's caller-stream and thread tests are tests/test_gpu_repair_callers.py's).  outs: up to four
    (device address, capacity) or None, in the order of REPAIR_OUTPUTS; table: (device address, words) of the per-record table or None.
    Returns RepairStats."""
    return _repair_call(lib().scfq_repair_buffers, "scfq_repair_buffers",
                        [ctypes.c_void_p(ptr1) if ptr1 else None, n1, ctypes.c_void_p(ptr2) if ptr2 else None, n2, 1, _opts_ref(opts),
                         ctypes.c_void_p(table[0]) if table else None, table[1] if table else 0] + _repair_outputs(outs) + [1])


def repair_host(data1, data2, opts=None, caps=None, table_cap=None, want=(True, True, True, True)):
    """fq-repair of two host buffers.  caps: the four capacities (None in it: that output is left out), or None: a sizing call first and
    then the outputs in `want` at their sizes; table_cap: the words of the per-record table (None: reads1 + reads2, 0: no table).
    Returns (RepairStats, table, [out1, out2, singles1, singles2]): table a numpy uint32 array or None, the outputs as bytes or None."""
    import numpy as np
    a1, n1, keep1 = _host_ptr(data1)
    a2, n2, keep2 = _host_ptr(data2)
    head = [a1, n1, a2, n2, 0, _opts_ref(opts)]
    fn = lib().scfq_repair_buffers
    if caps is None or table_cap is None:
        s = _repair_call(fn, "scfq_repair_buffers", head + [None, 0] + [None, 0] * 4 + [0])
        if caps is None:
            caps = [getattr(s, n + "_bytes") if w else None for n, w in zip(REPAIR_OUTPUTS, want)]
        if table_cap is None:
            table_cap = int(s.reads1 + s.reads2)
    table = np.zeros(max(table_cap, 1), dtype=np.uint32) if table_cap else None
    bufs = [None if c is None else ctypes.create_string_buffer(max(int(c), 1)) for c in caps]
    outs = [None if b is None else (ctypes.addressof(b), int(c)) for b, c in zip(bufs, caps)]
    s = _repair_call(fn, "scfq_repair_buffers", head + [table.ctypes.data if table_cap else None, table_cap] + _repair_outputs(outs) + [0])
    sizes = [getattr(s, n + "_bytes") for n in REPAIR_OUTPUTS]
    return s, (table[:int(s.reads1 + s.reads2)] if table_cap else None), [None if b is None else b.raw[:int(k)] for b, k in zip(bufs, sizes)]


def repair_files(path1, path2, opts=None, out1_fd=-1, out2_fd=-1, singles1_fd=-1, singles2_fd=-1, per_read_fd=-1):
    """A descriptor below 0: that output is not produced.  Returns RepairStats"""
    return _repair_call(lib().scfq_repair_files, "scfq_repair_files",
                        [os.fsencode(path1) if path1 is not None else None, os.fsencode(path2) if path2 is not None else None, _opts_ref(opts), None,
                         out1_fd, out2_fd, singles1_fd, singles2_fd, per_read_fd])


def format_repair_stats_tsv(s, header=False):
    buf = ctypes.create_string_buffer(1024)
    n = lib().scfq_format_repair_stats_tsv(ctypes.byref(s) if s is not None else None, 1 if header else 0, buf, 1024)
    if n < 0:
        raise ScfqError(n, "scfq_format_repair_stats_tsv")
    return buf.value.decode()


def format_repair_rec_tsv(which, record=0, mate=SCFQ_REPAIR_SINGLE):
    """which: 1 or 2, the input of the record; 0: the column names"""
    buf = ctypes.create_string_buffer(96)
    lib().scfq_format_repair_rec_tsv(which, record, mate, buf, 96)
    return buf.value.decode()


def repair_stages():
    """(line indexes, P1, the positional check, P2, sort, rounds, mates, lengths with their scans, W1 + W2) milliseconds of this thread's last
    fq-repair call; all but the first are HIP-event times, zeros unless SCFQ_REPAIR_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 9)()
    lib().scfq_debug_repair_stages(ms, 9)
    return list(ms)


def _fa_check(rc, what):
    if rc != 0:
        raise ScfqError(rc, what, lib().scfq_fa_error_detail().decode() or lib().scfq_last_error_detail().decode())


class FaIndex:
    """scfq_fa_index: the tile tables of one FASTA on the device and its contig table.  `summary` is the FaSummary of the
    indexing call, `contigs` a list of (name, header_offset, length) in file order.  A device buffer that was indexed in
    place stays the caller's and has to outlive the index.  close() (or the end of a `with`) frees it."""

    def __init__(self, handle, summary, keep=None):
        self._h, self.summary, self._keep = handle, summary, keep
        self.contigs = []
        c = FaContig()
        for i in range(summary.contigs):
            _fa_check(lib().scfq_fa_contig_at(self._h, i, ctypes.byref(c)), "scfq_fa_contig_at")
            self.contigs.append((ctypes.string_at(c.name, c.name_len).decode("latin-1"), c.header_offset, c.length))

    def find(self, name):
        """index of the first contig of that name, or None"""
        i = ctypes.c_uint64()
        raw = name.encode("latin-1") if isinstance(name, str) else name
        if b"\0" in raw:
            return None
        return i.value if lib().scfq_fa_contig_find(self._h, raw, ctypes.byref(i)) == 0 else None

    def close(self):
        if self._h:
            lib().scfq_fa_index_free(self._h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _fa_index_call(fn, what, keep, *head):
    h = ctypes.c_void_p()
    s = FaSummary()
    s.struct_size = ctypes.sizeof(FaSummary)
    _fa_check(fn(*head, ctypes.byref(h), ctypes.byref(s)), what)
    return FaIndex(h, s, keep)


def fa_index_device(dev_ptr, n):
    """fa-gc index of a device-resident FASTA (any alignment); the buffer stays the caller's and must outlive the index"""
    return _fa_index_call(lib().scfq_fa_index_buffer, "scfq_fa_index_buffer", None, ctypes.c_void_p(dev_ptr), n, 1)


def fa_index_host(data):
    """fa-gc index of a host buffer (bytes / numpy uint8): staged, the copy is owned by the index"""
    addr, n, keep = _host_ptr(data)
    return _fa_index_call(lib().scfq_fa_index_buffer, "scfq_fa_index_buffer", None, addr, n, 0)


def fa_index_file(path):
    return _fa_index_call(lib().scfq_fa_index_file, "scfq_fa_index_file", None, os.fsencode(path), None)


def fa_count_intervals(index, intervals):
    """intervals: (contig, begin, end) rows, 0-based and half-open (a list, or a numpy uint64 array of shape (nq, 3)).
    Returns a numpy uint64 array of shape (nq, 3): gc, acgt, bases."""
    import numpy as np
    q = np.ascontiguousarray(np.asarray(intervals, dtype=np.uint64).reshape(-1, 3))
    out = np.zeros((q.shape[0], 3), dtype=np.uint64)
    _fa_check(lib().scfq_fa_count_intervals(index._h, q.ctypes.data if q.size else None, q.shape[0], out.ctypes.data if q.size else None),
              "scfq_fa_count_intervals")
    return out


def fa_parse_window(text):
    """sci_parse_int (helpers.nim:230-237) and the ">= 1" rule: "3,200" -> 3200, "1e3" -> 1000, "5e5" -> 312500000"""
    w = ctypes.c_uint64()
    _fa_check(lib().scfq_fa_parse_window(text.encode(), ctypes.byref(w)), "scfq_fa_parse_window")
    return w.value


def fa_gc_interval(pos, window, length):
    """(begin, end) of the bases a window around the 1-based pos covers, or None when pos is out of range"""
    b, e, bad = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    _fa_check(lib().scfq_fa_gc_interval(pos, window, length, ctypes.byref(b), ctypes.byref(e), ctypes.byref(bad)), "scfq_fa_gc_interval")
    return None if bad.value else (b.value, e.value)


def format_fa_gc_value(gc, acgt, window):
    buf = ctypes.create_string_buffer(64)
    _check(min(0, lib().scfq_format_fa_gc_value(gc, acgt, window, buf, 64)), "scfq_format_fa_gc_value")
    return buf.value.decode()


def fa_stages():
    """(F1 tile scan, F2 record scan, F3 contig table, 0) milliseconds of this thread's last fa index call: HIP-event times,
    zeros unless SCFQ_FA_TIMING=1 is in the environment"""
    ms = (ctypes.c_double * 4)()
    lib().scfq_debug_fa_stages(ms, 4)
    return list(ms)


SCFQ_META_WHOLE_FILE = 0x1


def meta_header():
    return lib().scfq_meta_header().decode()


def meta_file_tsv(path, sample_n=100, flags=0):
    """the 16-column fq-meta row of `path` (reference: src/fq_meta.nim:197-278)"""
    buf = ctypes.create_string_buffer(4096)
    _check(min(0, lib().scfq_meta_file_tsv(os.fsencode(path), sample_n, flags, buf, 4096)), "scfq_meta_file_tsv")
    return buf.value.decode()


def debug_bgzf_inflate(image, cap):
    """device-side inflate of a BGZF image held in host memory (bytes) -> bytes"""
    addr, n, keep = _host_ptr(image)
    out = (ctypes.c_uint8 * max(cap, 1))()
    r = lib().scfq_debug_bgzf_inflate(addr, n, out, cap)
    if r < 0:
        raise ScfqError(int(r), "scfq_debug_bgzf_inflate", lib().scfq_last_error_detail().decode())
    return ctypes.string_at(out, r)


def hist_stats():
    """(ranges served by the speculative K3 form, ranges (re)done by the exact kernel) of this thread's last histogram session"""
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    lib().scfq_debug_hist_stats(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def partial_simple_device(dev_ptr, n, prev_byte=-1):
    p = Partial()
    _check(lib().scfq_debug_partial_simple(ctypes.c_void_p(dev_ptr), n, prev_byte, ctypes.byref(p)),
           "scfq_debug_partial_simple")
    return p


def debug_gz_resume(path, after_bytes, cap, chunk_bytes=0):
    """host only: a gzip file's bytes with the first member read in two halves (serial decoder, then the mid-member take-over)"""
    buf = ctypes.create_string_buffer(max(cap, 1))
    n = lib().scfq_debug_gz_resume(os.fsencode(path), after_bytes, buf, cap, chunk_bytes)
    if n < 0:
        raise ScfqError(int(n), "scfq_debug_gz_resume", lib().scfq_last_error_detail().decode())
    return buf.raw[:n]


def debug_read_file(path, cap, chunk_bytes=0):
    """host-only: the byte stream count_file would scan (plain / BGZF parallel inflate / serial gzread)"""
    buf = (ctypes.c_uint8 * max(cap, 1))()
    n = lib().scfq_debug_read_file(os.fsencode(path), buf, cap, chunk_bytes)
    if n < 0:
        raise ScfqError(int(n), "scfq_debug_read_file", lib().scfq_last_error_detail().decode())
    return bytes(buf[:n])


def debug_stream_ms(dev_ptr, n, reps=5):
    """diagnostic: ms for the scan kernel's load structure alone (4 KiB-aligned device pointer)"""
    return lib().scfq_debug_stream_ms(ctypes.c_void_p(dev_ptr), n, reps)


def debug_last_scan_kernel():
    """diagnostic: the scan kernel instance + range geometry of this thread's last launch, e.g.
    'fq_scan_tiles<false, 0, 2, true, false> tiles_per_range=100/50/25/12': the range size of every segment of the launch
    (big ranges first, small ranges last), a single number for a uniform launch (histogram forms, small inputs, SCFQ_TAPER_WAVES=0)"""
    L = lib()
    L.scfq_debug_last_scan_kernel.restype = ctypes.c_int64
    L.scfq_debug_last_scan_kernel.argtypes = [ctypes.c_char_p, ctypes.c_uint64]
    buf = ctypes.create_string_buffer(256)
    L.scfq_debug_last_scan_kernel(buf, 256)
    return buf.value.decode()


class ScanGeometry(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_segments", ctypes.c_uint32), ("n_tiles", ctypes.c_uint64), ("n_ranges", ctypes.c_uint64),
                ("first_range", ctypes.c_uint64 * 6), ("first_tile", ctypes.c_uint64 * 6), ("tiles_per_range", ctypes.c_uint64 * 6)]

    def segments(self):
        """[(first_range, first_tile, tiles_per_range)] of the segments in force"""
        return [(int(self.first_range[s]), int(self.first_tile[s]), int(self.tiles_per_range[s])) for s in range(self.n_segments)]


def debug_scan_geometry(n, ptr_offset=0, flags=0, n_cu=0):
    """diagnostic, no device needed: the ranges a scan launch over n bytes starting ptr_offset bytes past a 4 KiB boundary would use
    (SCFQ_TILES_PER_RANGE and SCFQ_TAPER_WAVES of the environment apply)"""
    L = lib()
    L.scfq_debug_scan_geometry.restype = ctypes.c_int
    L.scfq_debug_scan_geometry.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ScanGeometry)]
    g = ScanGeometry()
    g.struct_size = ctypes.sizeof(ScanGeometry)
    _check(L.scfq_debug_scan_geometry(n, ptr_offset, flags, n_cu, ctypes.byref(g)), "scfq_debug_scan_geometry")
    return g


def combine(acc, b, hist_acc=None, hist_b=None):
    _check(lib().scfq_partial_combine(ctypes.byref(acc), ctypes.byref(b),
                                      ctypes.byref(hist_acc) if hist_acc is not None else None,
                                      ctypes.byref(hist_b) if hist_b is not None else None), "scfq_partial_combine")
    return acc


def identity():
    p = Partial()
    lib().scfq_partial_identity(ctypes.byref(p), None)
    return p


def finalize(p, hist=None):
    c = _new_counts()
    _check(lib().scfq_partial_finalize(ctypes.byref(p), ctypes.byref(hist) if hist is not None else None,
                                       ctypes.byref(c)), "scfq_partial_finalize")
    return c


def format_tsv(c):
    buf = ctypes.create_string_buffer(256)
    lib().scfq_format_tsv(ctypes.byref(c), buf, 256)
    return buf.value.decode()


def last_timing():
    t = Timing()
    t.struct_size = ctypes.sizeof(Timing)
    _check(lib().scfq_last_timing(ctypes.byref(t)), "scfq_last_timing")
    return t


SCFQ_SYNTH_ILLUMINA, SCFQ_SYNTH_NANOPORE = 0, 1


def synth_plan(kind, seed, min_bytes, first_record=0):
    info = SynthInfo()
    info.struct_size = ctypes.sizeof(SynthInfo)
    _check(lib().scfq_synth_plan(kind, seed, first_record, min_bytes, ctypes.byref(info)), "scfq_synth_plan")
    return info


def synth_locate(kind, seed, offset):
    rec, start = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().scfq_synth_locate(kind, seed, offset, ctypes.byref(rec), ctypes.byref(start)), "scfq_synth_locate")
    return rec.value, start.value


def synth_host(kind, seed, records, first_record=0):
    import numpy as np
    plan = SynthInfo()
    plan.struct_size = ctypes.sizeof(SynthInfo)
    # upper bound on size: plan with records via a dry call (dst NULL, cap 0 returns bytes needed)
    _check(lib().scfq_synth_host(kind, seed, first_record, records, None, 0, ctypes.byref(plan)), "scfq_synth_host")
    out = np.empty(plan.bytes, dtype=np.uint8)
    info = SynthInfo()
    info.struct_size = ctypes.sizeof(SynthInfo)
    _check(lib().scfq_synth_host(kind, seed, first_record, records, out.ctypes.data, out.size, ctypes.byref(info)),
           "scfq_synth_host")
    return out, info


def synth_device(kind, seed, records, dev_ptr, cap, first_record=0):
    info = SynthInfo()
    info.struct_size = ctypes.sizeof(SynthInfo)
    _check(lib().scfq_synth_device(kind, seed, first_record, records, ctypes.c_void_p(dev_ptr), cap,
                                   ctypes.byref(info)), "scfq_synth_device")
    return info


# ---------------------------------------------------------------------------------------------
# Python mirror of the reference operator (same names, argument meaning and error behaviour)
# ---------------------------------------------------------------------------------------------
fq_count_header = "\t".join(["reads", "gc_content", "gc_bases", "n_bases", "bases"])   # src/fq_count.nim:7-11


def output_header(header, basename, absolute):
    """src/utils/helpers.nim:200-208"""
    return "\t".join([x for x in (header, "basename" if basename else "", "absolute" if absolute else "") if x])


def get_absolute(path):
    """src/utils/helpers.nim:210-213 — symlinks: absolutePath(expandSymlink(path)) (relative targets resolve
    against the CWD, a reference quirk kept here)."""
    if os.path.islink(path):
        return os.path.abspath(os.readlink(path))
    return os.path.abspath(path)


def last_path_part(path):
    """Nim os.lastPathPart: tail of the path after stripping trailing separators."""
    return os.path.basename(path.rstrip("/")) if path.rstrip("/") else ""


def output_w_fnames(line, path, basename, absolute):
    """src/utils/helpers.nim:215-224"""
    parts = [line, last_path_part(path) if basename else "", get_absolute(path) if absolute else ""]
    return "\t".join([x for x in parts if x])


def error_msg(msg, error_code=1, stream=None):
    """src/utils/helpers.nim:29-30 (colorize fgRed)"""
    (stream or sys.stderr).write("\x1b[31mError %d: %s\x1b[0m\n" % (error_code, msg))


def quit_error(msg, error_code=1):
    """src/utils/helpers.nim:32-34"""
    error_msg(msg, error_code)
    sys.exit(error_code)


def fq_count(fastq, basename=False, absolute=False, out=None, flags=0, devices=None):
    """proc fq_count*(fastq: string, basename: bool, absolute: bool)   (src/fq_count.nim:14-53)

    Prints one TSV row. Unopenable input -> "Error 2: Unable to open file: <path>" and exit status 2
    (src/fq_count.nim:35-36). Paths shorter than 3 characters raise like the reference's
    fastq[^3 .. ^1] slice does (IndexError there; surfaces as exit 1 through sc.nim:299-305).
    """
    if len(fastq) < 3:
        raise IndexError("index out of bounds")   # fastq[^3 .. ^1], src/fq_count.nim:31
    try:
        c = count_file(fastq, flags=flags, devices=devices)
    except ScfqError as e:
        if e.rc == SCFQ_EOPEN:
            quit_error("Unable to open file: " + fastq, 2)
        raise
    (out or sys.stdout).write(output_w_fnames(format_tsv(c), fastq, basename, absolute) + "\n")
    return c


def warning_msg(msg, stream=None):
    """src/utils/helpers.nim:36-37 (colorize fgYellow)"""
    (stream or sys.stderr).write("\x1b[33mWarning: %s\x1b[0m\n" % msg)


def _fa_int(text):
    import re
    return int(text) if re.fullmatch(r"[+-]?[0-9]{1,18}", text) else None


def fa_positions(pos_in, err=None):
    """iter_pos (helpers.nim:88-151): [(chrom, pos)] of one "chr:pos" string or of a text file whose first two fields are
    chrom and position; warnings for the lines that are neither go to `err`"""
    import re
    if ":" in pos_in and "/" not in pos_in:
        chrom, _, pos = pos_in.partition(":")
        if _fa_int(pos) is None:
            quit_error("Invalid position: " + pos_in, 1)
        return [(chrom, _fa_int(pos))]
    if pos_in.lower().endswith(".bcf"):
        quit_error("BCF position files are not supported: " + pos_in + " (give chr:pos, or a text file: BED, VCF, TSV)", 1)
    try:
        if pos_in.endswith(".gz"):
            import gzip
            with gzip.open(pos_in, "rb") as f:
                text = f.read()
        else:
            with open(pos_in, "rb") as f:
                text = f.read()
    except OSError:
        quit_error("Unable to open file: " + pos_in, 2)
    out = []
    lines = text.decode("latin-1").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for n, line in enumerate(lines, 1):
        if line.endswith("\r"):
            line = line[:-1]
        fields = re.split(r"[\t: ]+", line.strip("\t: "))
        pos = _fa_int(fields[1]) if len(fields) >= 2 else None
        if pos is not None:
            out.append((fields[0], pos))
        elif n != 1 and not line.startswith("#"):
            warning_msg('Invalid line: %d in "%s" > %s' % (n, pos_in, line), err)
    return out


def fa_sort_key(chrom, pos):
    """The order of fa-gc's rows (see cli/sc_main.cpp): all-digit names by value and position, then x, y, m by that rank and
    position, then the other names; names lower-cased and without a leading "chr".  For sorted(), which is stable."""
    s = chrom.lower()
    if len(s) > 3 and s.startswith("chr"):
        s = s[3:]
    if all(c in "0123456789" for c in s):
        return (0, int(s or "0"), "", pos)
    if s in ("x", "y", "m"):
        return (1, "xym".index(s), "", pos)
    return (2, 0, s.encode("latin-1"), 0)


def fa_gc(fasta, positions_in, windows_in, out=None, err=None):
    """proc fa_gc*(fasta: string, positions_in: string, windows_in: seq[string])   (src/fa_gc.nim:59-100), as `sc fa-gc`
    prints it; returns the text (and writes it to `out` when given).  Every cell goes to the device in one call."""
    windows = []
    for w in windows_in:
        try:
            windows.append(fa_parse_window(w))
        except ScfqError as e:
            quit_error(lib().scfq_fa_error_detail().decode() or str(e), 1)
    positions = sorted(fa_positions(positions_in, err), key=lambda p: fa_sort_key(*p))
    try:
        index = fa_index_file(fasta)
    except ScfqError as e:
        if e.rc == SCFQ_EOPEN:
            quit_error("Unable to open file: " + fasta, 2)
        raise
    with index:
        text = ["\t".join(["chrom", "pos"] + ["gc_%d" % (2 * w) for w in windows])]
        rows, cells = [], []
        for chrom, pos in positions:
            c = index.find(chrom)
            spans = None if c is None else [fa_gc_interval(pos, w, index.contigs[c][2]) for w in windows]
            if spans is None or spans[0] is None:
                warning_msg("<%s:%d> is out of range" % (chrom, pos), err)
                continue
            rows.append((chrom, pos))
            cells += [(c, b, e) for b, e in spans]
        counts = fa_count_intervals(index, cells)
    for r, (chrom, pos) in enumerate(rows):
        vals = [format_fa_gc_value(int(counts[r * len(windows) + k][0]), int(counts[r * len(windows) + k][1]), w)
                for k, w in enumerate(windows)]
        text.append("\t".join([chrom, str(pos)] + vals))
    text = "\n".join(text) + "\n"
    if out is not None:
        out.write(text)
    return text
