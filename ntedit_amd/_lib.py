"""ctypes binding of include/ntedit_hip.h (libntedit_hip.so, built in-tree).

There is deliberately no fallback: if the HIP library is missing or no GPU is
visible, every compute call raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NTEDIT_HIP_LIB") or os.path.join(_HERE, "libntedit_hip.so")  # (override: A/B builds)


class NtEditHipError(RuntimeError):
    pass


class Params(ctypes.Structure):
    """ntedit_hip_params (the reference's opt:: block, ntedit.cpp:99-133)."""
    _fields_ = [
        ("min_contig_len", ctypes.c_uint32),
        ("max_insertions", ctypes.c_uint32),
        ("max_deletions", ctypes.c_uint32),
        ("edit_threshold", ctypes.c_float),
        ("missing_threshold", ctypes.c_float),
        ("edit_ratio", ctypes.c_float),
        ("missing_ratio", ctypes.c_float),
        ("use_ratio", ctypes.c_int32),
        ("jump", ctypes.c_uint32),
        ("mode", ctypes.c_int32),
        ("snv", ctypes.c_int32),
        ("mask", ctypes.c_int32),
        ("min_threshold", ctypes.c_uint32),
        ("max_threshold", ctypes.c_uint32),
        ("start_grid", ctypes.c_uint32),
        ("node_window", ctypes.c_uint32),
        ("screen_mode", ctypes.c_uint32),
        ("event_budget", ctypes.c_uint32),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("bases", ctypes.c_uint64),
        ("absent_kmers", ctypes.c_uint64),
        ("events", ctypes.c_uint64),
        ("events_deferred", ctypes.c_uint64),
        ("events_applied", ctypes.c_uint64),
        ("substitutions", ctypes.c_uint64),
        ("insertions", ctypes.c_uint64),
        ("deletions", ctypes.c_uint64),
        ("ms_screen", ctypes.c_float),
        ("ms_extract", ctypes.c_float),
        ("ms_machine", ctypes.c_float),
        ("ms_total", ctypes.c_float),
        ("screen_launches", ctypes.c_uint32),
        ("screen_binned", ctypes.c_uint32),
        ("ms_partition", ctypes.c_float),
        ("ms_probe", ctypes.c_float),
        ("events_skipped", ctypes.c_uint32),
        ("screen_chunks_direct", ctypes.c_uint32),
        ("screen_overflow_records", ctypes.c_uint64),
    ]


class ReadsPassStats(ctypes.Structure):
    """ntedit_hip_reads_pass_stats"""
    _fields_ = [("bases", ctypes.c_uint64), ("ms_wall", ctypes.c_double), ("ms_gpu", ctypes.c_double)]


MERGE_SAT_ADD, MERGE_OR, MERGE_MAX = 0, 1, 2
READS_PASS_COUNT, READS_PASS_HIST, READS_PASS_SOLID = 0, 1, 2
RESIDENT_OFF, RESIDENT_ON, RESIDENT_OVER_CAP, RESIDENT_NO_MEMORY = 0, 1, 2, 3


class ResidentStats(ctypes.Structure):
    """ntedit_hip_resident_stats"""
    _fields_ = [("state", ctypes.c_int), ("batches", ctypes.c_uint64), ("bases", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64), ("cap", ctypes.c_uint64)]


READS_LOG_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p)


class ReadsBuildArgs(ctypes.Structure):
    """ntedit_hip_reads_build_args"""
    _fields_ = [("files", ctypes.POINTER(ctypes.c_char_p)), ("n_files", ctypes.c_uint32), ("k", ctypes.c_uint32),
                ("hash_num", ctypes.c_uint32), ("cmin", ctypes.c_uint32), ("solid", ctypes.c_int),
                ("counts", ctypes.c_int), ("bf_bytes", ctypes.c_uint64), ("fpr", ctypes.c_double),
                ("sketch_counters", ctypes.c_uint64), ("batch_bytes", ctypes.c_uint64), ("hist_path", ctypes.c_char_p),
                ("sketch_path", ctypes.c_char_p), ("use_store", ctypes.c_int), ("store_cap", ctypes.c_uint64),
                ("log", READS_LOG_FN), ("user", ctypes.c_void_p), ("begins", ctypes.POINTER(ctypes.c_uint64)),
                ("ends", ctypes.POINTER(ctypes.c_uint64)), ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32),
                ("device_parse", ctypes.c_int), ("reject_cmin", ctypes.c_uint32), ("reject_bf_bytes", ctypes.c_uint64),
                ("reject_num_elements", ctypes.c_uint64), ("min_read", ctypes.c_uint32), ("keep_store", ctypes.c_int),
                ("min_qual", ctypes.c_uint32)]


class ReadsBuildResult(ctypes.Structure):
    """ntedit_hip_reads_build_result"""
    _fields_ = [("cmin", ctypes.c_uint32), ("bf_bytes", ctypes.c_uint64), ("passes", ReadsPassStats * 3),
                ("store_state", ctypes.c_int), ("store_bytes", ctypes.c_uint64), ("ms_total", ctypes.c_double),
                ("store_batches", ctypes.c_uint64), ("reject_bf_bytes", ctypes.c_uint64),
                ("from_store", ctypes.c_int)]


# the reads-option rules (ntedit_hip_reads_options_check) and the header's defaults
READS_DIALECT_TOOL, READS_DIALECT_POLISHER = 0, 1
READS_REFUSED, READS_NOT_A_NUMBER, READS_EMPTY = 1, 2, 3
READS_BATCH_DEFAULT, READS_RESIDENT_CAP_DEFAULT, READS_GZIP_WEIGHT = 256 << 20, 48 << 30, 4
READS_OPTION_TEXTS = ("k", "cutoff", "hashes", "fpr", "bf", "num_elements", "sketch_bytes", "batch_bytes", "store_cap",
                      "threads")
READS_REJECT_OPTION_TEXTS = ("reject_cutoff", "reject_bf", "reject_num_elements")


class ReadsOptions(ctypes.Structure):
    """ntedit_hip_reads_options"""
    _fields_ = ([(name, ctypes.c_char_p) for name in READS_OPTION_TEXTS] +
                [("solid", ctypes.c_int), ("hist", ctypes.c_int), ("files", ctypes.POINTER(ctypes.c_char_p)),
                 ("n_files", ctypes.c_uint32), ("gpu_parse", ctypes.c_int)] +
                [(name, ctypes.c_char_p) for name in READS_REJECT_OPTION_TEXTS] +
                [("counts", ctypes.c_int), ("reject_out", ctypes.c_int), ("min_qual", ctypes.c_char_p)])


class ReadsRules(ctypes.Structure):
    """ntedit_hip_reads_rules"""
    _fields_ = [("k", ctypes.c_uint32), ("cmin", ctypes.c_uint32), ("hash_num", ctypes.c_uint32),
                ("fpr", ctypes.c_double), ("bf_bytes", ctypes.c_uint64), ("num_elements", ctypes.c_uint64),
                ("sketch_bytes", ctypes.c_uint64), ("sketch_counters", ctypes.c_uint64),
                ("batch_bytes", ctypes.c_uint64), ("store_cap", ctypes.c_uint64), ("threads", ctypes.c_uint64),
                ("gather_hist", ctypes.c_int), ("size_from_hist", ctypes.c_int), ("gpu_parse", ctypes.c_int),
                ("reject_cmin", ctypes.c_uint32), ("reject_bf_bytes", ctypes.c_uint64),
                ("reject_num_elements", ctypes.c_uint64), ("reject_size_from_hist", ctypes.c_int),
                ("min_qual", ctypes.c_uint32)]


READS_FILTER_OPTION_TEXTS = ("min_read_len", "min_mean_qual", "min_rq")


class ReadsFilterOptions(ctypes.Structure):
    """ntedit_hip_reads_filter_options: --min_read_len, --min_mean_qual, --min_rq as given (None: not given)"""
    _fields_ = [(name, ctypes.c_char_p) for name in READS_FILTER_OPTION_TEXTS]


class ReadsFilterRules(ctypes.Structure):
    """ntedit_hip_reads_filter_rules: what ntedit_hip_reads_filter_options_check makes of them (0: off)"""
    _fields_ = [("min_read_len", ctypes.c_uint32), ("min_mean_qual", ctypes.c_uint32), ("min_rq", ctypes.c_float)]


class ReadsReadFilterStats(ctypes.Structure):
    """ntedit_hip_reads_read_filter_stats: what the last pass's records came to under --min_read_len, --min_mean_qual, --min_rq"""
    _fields_ = [("records", ctypes.c_uint64), ("dropped_length", ctypes.c_uint64), ("dropped_rq", ctypes.c_uint64),
                ("dropped_mean_qual", ctypes.c_uint64), ("rq_tagged", ctypes.c_uint64), ("aux_malformed", ctypes.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# --gpu_parse (ntedit_hip_reads_parse_device / _model): the tile size and the rules of the clean grammar
PARSE_TILE = 16384
PARSE_BAD = dict(first=1, cr=2, empty=4, seq_start=8, fq_lines=16, fq_header=32, fq_plus=64, fq_qual=128, table=256,
                 size=512)


class ReadsParseResult(ctypes.Structure):
    """ntedit_hip_reads_parse_result"""
    _fields_ = [("clean", ctypes.c_int), ("broken", ctypes.c_uint32), ("kind", ctypes.c_int),
                ("text_len", ctypes.c_uint64), ("reads", ctypes.c_uint64), ("bases", ctypes.c_uint64),
                ("lines", ctypes.c_uint64)]


class SettleStats(ctypes.Structure):
    """ntedit_hip_settle_stats"""
    _fields_ = [("events_seen", ctypes.c_uint64), ("events_settled", ctypes.c_uint64), ("ms", ctypes.c_float)]


APPLY_EDITED, APPLY_QV, APPLY_SHARED, APPLY_BGZF, APPLY_TRACK = 1, 2, 4, 8, 16


class QvRow(ctypes.Structure):
    """ntedit_hip_qv_row: the QV counts of one entry of a batch polished with APPLY_QV"""
    _fields_ = [("len_before", ctypes.c_uint64), ("len_after", ctypes.c_uint64), ("kmers_before", ctypes.c_uint64),
                ("absent_before", ctypes.c_uint64), ("kmers_after", ctypes.c_uint64), ("absent_after", ctypes.c_uint64)]


QV_DTYPE = [(name, "<u8") for name, _ in QvRow._fields_]


class ApplyStats(ctypes.Structure):
    """ntedit_hip_apply_stats"""
    _fields_ = [("ms_apply", ctypes.c_float), ("ms_screen", ctypes.c_float), ("ms_count", ctypes.c_float),
                ("pieces", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("events_applied", ctypes.c_uint64)]


class BgzfStats(ctypes.Structure):
    """ntedit_hip_bgzf_stats: the context's last call that compressed (APPLY_BGZF, ntedit_hip_bgzf_deflate)"""
    _fields_ = [("ms_image", ctypes.c_float), ("ms_deflate", ctypes.c_float), ("ms_copy", ctypes.c_float),
                ("plain_bytes", ctypes.c_uint64), ("bgzf_bytes", ctypes.c_uint64), ("members", ctypes.c_uint32),
                ("stored_members", ctypes.c_uint32)]


BGZF_BLOCK = 65280  # plain bytes of a member


class TrackInterval(ctypes.Structure):
    """ntedit_hip_track_interval: one unsupported region of an entry (APPLY_TRACK, ntedit_hip_track_extract)"""
    _fields_ = [("entry", ctypes.c_uint32), ("begin", ctypes.c_uint32), ("end", ctypes.c_uint32),
                ("absent", ctypes.c_uint32)]


TRACK_DTYPE = [(name, "<u4") for name, _ in TrackInterval._fields_]


class TrackStats(ctypes.Structure):
    """ntedit_hip_track_stats: the context's last call that extracted intervals; [0] before, [1] after"""
    _fields_ = [("ms", ctypes.c_float * 2), ("intervals", ctypes.c_uint64 * 2), ("bases", ctypes.c_uint64 * 2)]


class DepthRow(ctypes.Structure):
    """ntedit_hip_depth_row: an entry's k-mer occurrences, the sum of their multiplicities and the saturated ones, before
    and after (ntedit_hip_set_spectrum)"""
    _fields_ = [("kmers_before", ctypes.c_uint64), ("sum_before", ctypes.c_uint64), ("saturated_before", ctypes.c_uint64),
                ("kmers_after", ctypes.c_uint64), ("sum_after", ctypes.c_uint64), ("saturated_after", ctypes.c_uint64)]


DEPTH_DTYPE = [(name, "<u8") for name, _ in DepthRow._fields_]
SPECTRUM_ROW_DTYPE = [("kmers", "<u8"), ("sum", "<u8"), ("saturated", "<u8")]  # ntedit_hip_spectrum_count's rows


class SpectrumStats(ctypes.Structure):
    """ntedit_hip_spectrum_stats: the context's last call that counted a spectrum; [0] before, [1] after"""
    _fields_ = [("ms", ctypes.c_float * 2), ("kmers", ctypes.c_uint64 * 2)]


class CnRow(ctypes.Structure):
    """ntedit_hip_cn_row: an entry's k-mer occurrences and those of assembly copy number 1, 2, 3, 4 and 5 or more on one
    side (ntedit_hip_set_cn)"""
    _fields_ = [("kmers", ctypes.c_uint64), ("cn1", ctypes.c_uint64), ("cn2", ctypes.c_uint64), ("cn3", ctypes.c_uint64),
                ("cn4", ctypes.c_uint64), ("cn5plus", ctypes.c_uint64)]


CN_ROW_DTYPE = [(name, "<u8") for name, _ in CnRow._fields_]
CN_OFF, CN_ON, CN_OVER_CAP, CN_NO_MEMORY = 0, 1, 2, 3
CN_STORE_DEFAULT = 32 << 30


class CnStats(ctypes.Structure):
    """ntedit_hip_cn_stats: the draft store and the last ntedit_hip_cn_finish; [0] before, [1] after; ms: k_cn_count
    before, k_spectrum_cn before, k_cn_count after, k_spectrum_cn after"""
    _fields_ = [("state", ctypes.c_uint32), ("finished", ctypes.c_uint32), ("batches", ctypes.c_uint64 * 2),
                ("bytes", ctypes.c_uint64 * 2), ("entries", ctypes.c_uint64 * 2), ("cap", ctypes.c_uint64),
                ("counters", ctypes.c_uint64), ("nonzero", ctypes.c_uint64 * 2), ("ms", ctypes.c_float * 4)]


class SharedStats(ctypes.Structure):
    """ntedit_hip_shared_stats: the popcounts behind the k-mer completeness (ntedit_hip_shared_counts)"""
    _fields_ = [("bits", ctypes.c_uint64), ("hash_num", ctypes.c_uint32), ("k", ctypes.c_uint32),
                ("filter_set", ctypes.c_uint64), ("shared_set", ctypes.c_uint64 * 2), ("marked_calls", ctypes.c_uint64),
                ("ms_mark", ctypes.c_float * 2)]


class ReadsParseStats(ctypes.Structure):
    """ntedit_hip_reads_parse_stats"""
    _fields_ = [("device_chunks", ctypes.c_uint64), ("fallback_chunks", ctypes.c_uint64),
                ("raw_bytes", ctypes.c_uint64), ("text_bytes", ctypes.c_uint64), ("ms_kernels", ctypes.c_double),
                ("broken", ctypes.c_uint32), ("host_files", ctypes.c_uint32)]


class BgzfMember(ctypes.Structure):
    """ntedit_hip_bgzf_member: one BGZF member of a buffer of compressed bytes"""
    _fields_ = [("in_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("n_in", ctypes.c_uint32),
                ("n_out", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ReadsInflateStats(ctypes.Structure):
    """ntedit_hip_reads_inflate_stats: --gpu_parse on BGZF inputs, the last pass of a context"""
    _fields_ = [("members", ctypes.c_uint64), ("comp_bytes", ctypes.c_uint64), ("raw_bytes", ctypes.c_uint64),
                ("ms_kernels", ctypes.c_double), ("files", ctypes.c_uint32), ("handed_back", ctypes.c_uint32),
                ("handed_back_at", ctypes.c_uint64), ("bad_member", ctypes.c_uint64), ("bad_reason", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


BGZF_END, BGZF_CUT, BGZF_NOT, BGZF_FULL = 0, 1, 2, 3


# --gpu_parse on BAM reads (ntedit_hip_reads_bam_device / _model): the default segment of the walk and the rules
BAM_SEGMENT = 8192
BAM_BAD_MAGIC, BAM_BAD_HEADER, BAM_BAD_RECORD, BAM_BAD_SIZE = 1, 2, 4, 8


class ReadsBamResult(ctypes.Structure):
    """ntedit_hip_reads_bam_result"""
    _fields_ = [("clean", ctypes.c_int), ("broken", ctypes.c_uint32), ("header_len", ctypes.c_uint64),
                ("n_ref", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("cut", ctypes.c_uint64),
                ("records", ctypes.c_uint64), ("kept", ctypes.c_uint64), ("skipped_flag", ctypes.c_uint64),
                ("skipped_short", ctypes.c_uint64), ("bases", ctypes.c_uint64), ("text_len", ctypes.c_uint64)]


class ReadsBamStats(ctypes.Structure):
    """ntedit_hip_reads_bam_stats: --gpu_parse on BAM inputs, since the context's last pass began"""
    _fields_ = [("files", ctypes.c_uint64), ("chunks", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("kept", ctypes.c_uint64), ("skipped_flag", ctypes.c_uint64), ("skipped_short", ctypes.c_uint64),
                ("segments", ctypes.c_uint64), ("rewalked", ctypes.c_uint64), ("ms_walk", ctypes.c_double),
                ("ms_decode", ctypes.c_double)]


# --gpu_parse for genome FASTA (ntedit_hip_genome_parse_device / _model): the entry and exit states of a chunk
GENOME_LINE_START, GENOME_IN_HEADER, GENOME_IN_SEQ = 0, 1, 2


class GenomeParseResult(ctypes.Structure):
    """ntedit_hip_genome_parse_result"""
    _fields_ = [("clean", ctypes.c_int), ("broken", ctypes.c_uint32), ("state_out", ctypes.c_int),
                ("reserved", ctypes.c_int), ("text_len", ctypes.c_uint64), ("bases", ctypes.c_uint64),
                ("lines", ctypes.c_uint64), ("last_header", ctypes.c_uint64)]


class GenomePassInfo(ctypes.Structure):
    """ntedit_hip_genome_pass_info: the last ntedit_hip_genome_pass of a context"""
    _fields_ = [("device_chunks", ctypes.c_uint64), ("raw_bytes", ctypes.c_uint64), ("text_bytes", ctypes.c_uint64),
                ("ms_kernels", ctypes.c_double), ("handed_back", ctypes.c_uint32), ("broken", ctypes.c_uint32),
                ("host_files", ctypes.c_uint32), ("bgzf_files", ctypes.c_uint32), ("bgzf_members", ctypes.c_uint64)]
READS_NO_START = 2 ** 64 - 1


class Segment(ctypes.Structure):
    """ntedit_hip_segment: a batch entry that is one segment of a contig cut for multi-GPU sharding"""
    _fields_ = [("pos_offset", ctypes.c_uint32), ("halo", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


SEG_NO_HEADER, SEG_NO_NEWLINE, SEG_SKIP = 1, 2, 4
E_ARG, E_SEGMENT = -1, -7
E_OVERFLOW = -4
EDIT_SUB, EDIT_INS, EDIT_DEL, EDIT_SNV_KEPT = 1, 2, 3, 4


class Edit(ctypes.Structure):
    """ntedit_hip_edit: one _changes.tsv row as a POD record"""
    _fields_ = [("contig", ctypes.c_uint32), ("draft_pos", ctypes.c_uint32), ("bases_off", ctypes.c_uint32),
                ("len", ctypes.c_uint16), ("support", ctypes.c_uint16), ("kind", ctypes.c_uint8),
                ("draft_base", ctypes.c_uint8), ("new_base", ctypes.c_uint8), ("n_alt", ctypes.c_uint8),
                ("alt_base", ctypes.c_uint8 * 3), ("alt_support", ctypes.c_uint8 * 3), ("reserved", ctypes.c_uint8 * 2)]


# the same record as a numpy dtype (28 bytes)
EDIT_DTYPE = [("contig", "<u4"), ("draft_pos", "<u4"), ("bases_off", "<u4"), ("len", "<u2"), ("support", "<u2"),
              ("kind", "u1"), ("draft_base", "u1"), ("new_base", "u1"), ("n_alt", "u1"), ("alt_base", "u1", (3,)),
              ("alt_support", "u1", (3,)), ("reserved", "u1", (2,))]


class WriteOptions(ctypes.Structure):
    """ntedit_hip_write_options"""
    _fields_ = [("fa_path", ctypes.c_char_p), ("tsv_path", ctypes.c_char_p), ("vcf_path", ctypes.c_char_p),
                ("append", ctypes.c_int), ("annot", ctypes.c_void_p), ("segments", ctypes.c_void_p),
                ("out_sizes", ctypes.c_void_p)]


# every symbol include/ntedit_hip.h declares
EXPORTS = [
    "ntedit_hip_params_default", "ntedit_hip_params_clamp", "ntedit_hip_create", "ntedit_hip_destroy",
    "ntedit_hip_last_error", "ntedit_hip_set_filter", "ntedit_hip_set_filter_device",
    "ntedit_hip_load_filter_file", "ntedit_hip_filter_info", "ntedit_hip_filter_device_ptr",
    "ntedit_hip_filter_alloc", "ntedit_hip_filter_insert", "ntedit_hip_filter_download",
    "ntedit_hip_filter_save_file", "ntedit_hip_set_params", "ntedit_hip_screen", "ntedit_hip_polish_batch",
    "ntedit_hip_result_free", "ntedit_hip_result_stats", "ntedit_hip_write_outputs",
    "ntedit_hip_write_tsv_header", "ntedit_hip_last_kernel_ms", "ntedit_hip_gather_bench",
    "ntedit_hip_annot_load", "ntedit_hip_annot_free", "ntedit_hip_write_vcf_header", "ntedit_hip_write_outputs_vcf",
    "ntedit_hip_set_host_threads", "ntedit_hip_filter_occupancy",
    "ntedit_hip_write_outputs_ex", "ntedit_hip_result_cover_ends", "ntedit_hip_result_edits",
    "ntedit_hip_host_alloc", "ntedit_hip_host_free", "ntedit_hip_bind_near_device", "ntedit_hip_set_tuning", "ntedit_hip_build_id", "ntedit_hip_device_tables", "ntedit_hip_packed_size", "ntedit_hip_pack_bases",
    "ntedit_hip_fasta_load", "ntedit_hip_fasta_open", "ntedit_hip_fasta_read", "ntedit_hip_fasta_count", "ntedit_hip_fasta_blob", "ntedit_hip_fasta_record",
    "ntedit_hip_fasta_free", "ntedit_hip_result_cuts_ok", "ntedit_hip_reserve",
    "ntedit_hip_sketch_alloc", "ntedit_hip_sketch_count", "ntedit_hip_sketch_occupancy", "ntedit_hip_sketch_download",
    "ntedit_hip_sketch_save_file", "ntedit_hip_sketch_free", "ntedit_hip_filter_alloc_counting",
    "ntedit_hip_filter_insert_solid", "ntedit_hip_reads_last_error", "ntedit_hip_sketch_histogram",
    "ntedit_hip_sketch_histogram_download", "ntedit_hip_reads_hist_summary", "ntedit_hip_reads_solid_cutoff",
    "ntedit_hip_sketch_set_device", "ntedit_hip_sketch_info", "ntedit_hip_merge_bytes", "ntedit_hip_reads_pass",
    "ntedit_hip_reads_range_text", "ntedit_hip_reads_bf_size", "ntedit_hip_reads_default_sketch",
    "ntedit_hip_reads_is_gzip", "ntedit_hip_reads_write_hist",
    "ntedit_hip_resident_begin", "ntedit_hip_resident_info", "ntedit_hip_resident_histogram",
    "ntedit_hip_resident_insert_solid", "ntedit_hip_resident_free", "ntedit_hip_reads_build",
    "ntedit_hip_reads_stage_count", "ntedit_hip_reads_stage_histogram", "ntedit_hip_reads_stage_decide",
    "ntedit_hip_reads_stage_insert", "ntedit_hip_reads_options_check",
    "ntedit_hip_reads_parse_device", "ntedit_hip_reads_parse_model", "ntedit_hip_reads_set_device_parse",
    "ntedit_hip_reads_parse_info", "ntedit_hip_reads_set_reject_cutoff",
    "ntedit_hip_bgzf_walk", "ntedit_hip_reads_inflate_device", "ntedit_hip_reads_inflate_model",
    "ntedit_hip_reads_last_record_start", "ntedit_hip_reads_last_start_device", "ntedit_hip_reads_inflate_info",
    "ntedit_hip_reads_is_bam", "ntedit_hip_reads_bam_device", "ntedit_hip_reads_bam_model",
    "ntedit_hip_reads_bam_set_segment", "ntedit_hip_reads_bam_info",
    "ntedit_hip_genome_parse_device", "ntedit_hip_genome_parse_model", "ntedit_hip_genome_pass",
    "ntedit_hip_genome_pass_get_info", "ntedit_hip_genome_pass_line",
    "ntedit_hip_sketch_reset", "ntedit_hip_resident_count", "ntedit_hip_reads_set_min_read",
    "ntedit_hip_settle_info",
    "ntedit_hip_reads_set_min_qual", "ntedit_hip_reads_min_qual_info", "ntedit_hip_reads_parse_model_q",
    "ntedit_hip_reads_bam_model_q", "ntedit_hip_reads_range_text_q",
    "ntedit_hip_reads_set_read_filter", "ntedit_hip_reads_get_read_filter", "ntedit_hip_reads_filter_options_check",
    "ntedit_hip_reads_read_filter_info", "ntedit_hip_reads_parse_model_f",
    "ntedit_hip_reads_bam_model_f", "ntedit_hip_reads_range_text_f", "ntedit_hip_reads_bam_set_group_width",
    "ntedit_hip_reads_bam_group_width",
    "ntedit_hip_set_apply", "ntedit_hip_result_edited_device", "ntedit_hip_result_edited",
    "ntedit_hip_result_last_error", "ntedit_hip_result_qv", "ntedit_hip_qv_value", "ntedit_hip_qv_header",
    "ntedit_hip_qv_format_row", "ntedit_hip_apply_info", "ntedit_hip_apply_tile",
    "ntedit_hip_shared_begin", "ntedit_hip_shared_reset", "ntedit_hip_shared_free", "ntedit_hip_shared_mark",
    "ntedit_hip_shared_download", "ntedit_hip_shared_counts", "ntedit_hip_bloom_cardinality",
    "ntedit_hip_completeness_header", "ntedit_hip_completeness_format_row",
    "ntedit_hip_set_fa_names", "ntedit_hip_result_fa_bgzf", "ntedit_hip_bgzf_deflate", "ntedit_hip_bgzf_deflate_model",
    "ntedit_hip_bgzf_bound", "ntedit_hip_bgzf_eof", "ntedit_hip_bgzf_info",
    "ntedit_hip_result_track", "ntedit_hip_track_extract", "ntedit_hip_track_info", "ntedit_hip_track_format_row",
    "ntedit_hip_set_spectrum", "ntedit_hip_result_spectrum", "ntedit_hip_result_depth", "ntedit_hip_spectrum_count",
    "ntedit_hip_spectrum_info", "ntedit_hip_spectrum_header", "ntedit_hip_spectrum_format_row", "ntedit_hip_depth_header",
    "ntedit_hip_depth_format_row",
    "ntedit_hip_set_cn", "ntedit_hip_cn_append", "ntedit_hip_cn_finish", "ntedit_hip_cn_table", "ntedit_hip_cn_rows",
    "ntedit_hip_cn_distinct", "ntedit_hip_cn_info", "ntedit_hip_cn_reset", "ntedit_hip_cn_free", "ntedit_hip_cn_header",
    "ntedit_hip_cn_format_row", "ntedit_hip_cn_contig_header", "ntedit_hip_cn_contig_format_row",
]
# ... and the declared names that hold a digit (a scan of the header for names of letters and underscores, as
# tests/test_abi.py makes one, does not see them)
EXPORTS_NUMBERED = ["ntedit_hip_filter_insert_solid2", "ntedit_hip_resident_insert_solid2"]

_lib = None


def load():
    """Load libntedit_hip.so; raises NtEditHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NtEditHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C ntedit_amd/csrc). There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.ntedit_hip_params_default.argtypes = [ctypes.POINTER(Params)]
    lib.ntedit_hip_params_default.restype = None
    lib.ntedit_hip_params_clamp.argtypes = [ctypes.POINTER(Params), ctypes.c_char_p, ctypes.c_size_t]
    lib.ntedit_hip_params_clamp.restype = None
    lib.ntedit_hip_create.argtypes = [ci, ctypes.POINTER(vp)]
    lib.ntedit_hip_destroy.argtypes = [vp]
    lib.ntedit_hip_destroy.restype = None
    lib.ntedit_hip_last_error.argtypes = [vp]
    lib.ntedit_hip_last_error.restype = ctypes.c_char_p
    lib.ntedit_hip_set_filter.argtypes = [vp, ci, vp, u64, u32, u32, ci]
    lib.ntedit_hip_set_filter_device.argtypes = [vp, ci, vp, u64, u32, u32, ci]
    lib.ntedit_hip_load_filter_file.argtypes = [vp, ci, ctypes.c_char_p]
    lib.ntedit_hip_filter_info.argtypes = [vp, ci, ctypes.POINTER(u32), ctypes.POINTER(u32),
                                           ctypes.POINTER(u64), ctypes.POINTER(ci)]
    lib.ntedit_hip_filter_device_ptr.argtypes = [vp, ci]
    lib.ntedit_hip_filter_device_ptr.restype = vp
    lib.ntedit_hip_filter_alloc.argtypes = [vp, ci, u64, u32, u32]
    lib.ntedit_hip_filter_insert.argtypes = [vp, ci, vp, u64, ci]
    lib.ntedit_hip_filter_download.argtypes = [vp, ci, vp]
    lib.ntedit_hip_filter_save_file.argtypes = [vp, ci, ctypes.c_char_p]
    lib.ntedit_hip_set_params.argtypes = [vp, ctypes.POINTER(Params)]
    lib.ntedit_hip_screen.argtypes = [vp, vp, u64, ci, vp]
    lib.ntedit_hip_polish_batch.argtypes = [vp, vp, u64, vp, vp, u32, ci, ctypes.POINTER(vp)]
    lib.ntedit_hip_result_free.argtypes = [vp]
    lib.ntedit_hip_result_free.restype = None
    lib.ntedit_hip_result_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.ntedit_hip_write_outputs.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_char_p), u32,
                                             ctypes.c_char_p, ctypes.c_char_p, ci]
    lib.ntedit_hip_write_tsv_header.argtypes = [ctypes.c_char_p, u32, u32, ci]
    lib.ntedit_hip_annot_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    lib.ntedit_hip_annot_free.argtypes = [vp]
    lib.ntedit_hip_annot_free.restype = None
    lib.ntedit_hip_write_vcf_header.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.ntedit_hip_write_outputs_vcf.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_char_p), u32,
                                                 ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ci, ci, vp]
    lib.ntedit_hip_write_outputs_ex.argtypes = [vp, vp, vp, vp, ctypes.POINTER(ctypes.c_char_p), u32,
                                                ctypes.POINTER(WriteOptions)]
    lib.ntedit_hip_result_cover_ends.argtypes = [vp, u32, vp]
    lib.ntedit_hip_result_edits.argtypes = [vp, vp, vp, vp, u32, vp, ctypes.POINTER(vp), ctypes.POINTER(u64),
                                            ctypes.POINTER(vp)]
    lib.ntedit_hip_host_alloc.argtypes = [ctypes.c_size_t]
    lib.ntedit_hip_host_alloc.restype = vp
    lib.ntedit_hip_host_free.argtypes = [vp]
    lib.ntedit_hip_host_free.restype = None
    lib.ntedit_hip_bind_near_device.argtypes = [ci]
    lib.ntedit_hip_filter_occupancy.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.ntedit_hip_set_host_threads.argtypes = [ctypes.c_uint]
    lib.ntedit_hip_set_host_threads.restype = None
    lib.ntedit_hip_last_kernel_ms.argtypes = [vp]
    lib.ntedit_hip_last_kernel_ms.restype = ctypes.c_float
    lib.ntedit_hip_gather_bench.argtypes = [vp, u64, u64, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_float)]
    lib.ntedit_hip_set_tuning.argtypes = [vp, ctypes.c_char_p, u64]
    lib.ntedit_hip_packed_size.argtypes = [u64]
    lib.ntedit_hip_packed_size.restype = u64
    lib.ntedit_hip_pack_bases.argtypes = [vp, u64, vp, ctypes.c_uint]
    lib.ntedit_hip_build_id.argtypes = []
    lib.ntedit_hip_build_id.restype = ctypes.c_char_p
    lib.ntedit_hip_reserve.argtypes = [vp, u64, u32, u64, ci]
    lib.ntedit_hip_result_cuts_ok.argtypes = [vp, u32, vp, vp, vp]
    lib.ntedit_hip_fasta_load.argtypes = [ctypes.c_char_p, u64, ctypes.c_uint, ctypes.POINTER(vp), ctypes.c_char_p,
                                          ctypes.c_size_t]
    lib.ntedit_hip_fasta_open.argtypes = lib.ntedit_hip_fasta_load.argtypes
    lib.ntedit_hip_fasta_read.argtypes = [vp, u64, u64, u64, vp]
    lib.ntedit_hip_fasta_count.argtypes = [vp]
    lib.ntedit_hip_fasta_count.restype = u64
    lib.ntedit_hip_fasta_blob.argtypes = [vp, ctypes.POINTER(u64)]
    lib.ntedit_hip_fasta_blob.restype = vp
    lib.ntedit_hip_fasta_record.argtypes = [vp, u64, ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(u64),
                                            ctypes.POINTER(u64)]
    lib.ntedit_hip_fasta_free.argtypes = [vp]
    lib.ntedit_hip_fasta_free.restype = None
    # reads k-mer filter build (ntedit-make-reads-bf)
    lib.ntedit_hip_sketch_alloc.argtypes = [vp, u64, u32, u32]
    lib.ntedit_hip_sketch_count.argtypes = [vp, vp, u64, ci]
    lib.ntedit_hip_sketch_occupancy.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.ntedit_hip_sketch_download.argtypes = [vp, vp]
    lib.ntedit_hip_sketch_save_file.argtypes = [vp, ctypes.c_char_p]
    lib.ntedit_hip_sketch_free.argtypes = [vp]
    lib.ntedit_hip_sketch_free.restype = None
    lib.ntedit_hip_filter_alloc_counting.argtypes = [vp, ci, u64, u32, u32]
    lib.ntedit_hip_filter_insert_solid.argtypes = [vp, ci, vp, u64, ci, u32]
    lib.ntedit_hip_reads_last_error.argtypes = [vp]
    lib.ntedit_hip_reads_last_error.restype = ctypes.c_char_p
    lib.ntedit_hip_sketch_histogram.argtypes = [vp, vp, u64, ci]
    lib.ntedit_hip_sketch_histogram_download.argtypes = [vp, vp]
    lib.ntedit_hip_reads_hist_summary.argtypes = [vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.ntedit_hip_reads_solid_cutoff.argtypes = [vp, ctypes.POINTER(u32)]
    pu64 = ctypes.POINTER(u64)
    lib.ntedit_hip_sketch_set_device.argtypes = [vp, vp, u64, u32, u32]
    lib.ntedit_hip_sketch_info.argtypes = [vp, pu64, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.ntedit_hip_merge_bytes.argtypes = [vp, vp, vp, u32, u64, ci]
    lib.ntedit_hip_reads_pass.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p), pu64, pu64, u32, u64, u32,
                                          ctypes.POINTER(ReadsPassStats), pu64, pu64]
    lib.ntedit_hip_reads_range_text.argtypes = [ctypes.c_char_p, u64, u64, vp, u64, pu64, pu64, pu64, pu64]
    lib.ntedit_hip_reads_bf_size.argtypes = [u64, u32, ctypes.c_double]
    lib.ntedit_hip_reads_bf_size.restype = u64
    lib.ntedit_hip_reads_default_sketch.argtypes = [ctypes.POINTER(ctypes.c_char_p), u32, u64]
    lib.ntedit_hip_reads_default_sketch.restype = u64
    lib.ntedit_hip_reads_is_gzip.argtypes = [ctypes.c_char_p]
    lib.ntedit_hip_reads_write_hist.argtypes = [ctypes.c_char_p, vp, u64, u64]
    # the resident store and the shared build (ntedit --reads)
    lib.ntedit_hip_resident_begin.argtypes = [vp, u64]
    lib.ntedit_hip_resident_info.argtypes = [vp, ctypes.POINTER(ResidentStats)]
    lib.ntedit_hip_resident_histogram.argtypes = [vp]
    lib.ntedit_hip_resident_insert_solid.argtypes = [vp, ci, u32]
    lib.ntedit_hip_resident_free.argtypes = [vp]
    lib.ntedit_hip_resident_free.restype = None
    args, res = ctypes.POINTER(ReadsBuildArgs), ctypes.POINTER(ReadsBuildResult)
    lib.ntedit_hip_reads_build.argtypes = [vp, args, res]
    lib.ntedit_hip_reads_stage_count.argtypes = [vp, args, res, pu64, pu64]
    lib.ntedit_hip_reads_stage_histogram.argtypes = [vp, args, res, vp]
    lib.ntedit_hip_reads_stage_decide.argtypes = [args, vp, res]
    lib.ntedit_hip_reads_stage_insert.argtypes = [vp, args, res]
    lib.ntedit_hip_reads_options_check.argtypes = [ctypes.POINTER(ReadsOptions), ci, ci, ctypes.POINTER(ReadsRules)]
    # --gpu_parse
    pres = ctypes.POINTER(ReadsParseResult)
    lib.ntedit_hip_reads_parse_device.argtypes = [vp, vp, u64, ci, u32, vp, u64, pres]
    lib.ntedit_hip_reads_parse_model.argtypes = [vp, u64, u32, vp, u64, pres]
    lib.ntedit_hip_reads_set_device_parse.argtypes = [vp, ci]
    lib.ntedit_hip_reads_parse_info.argtypes = [vp, ctypes.POINTER(ReadsParseStats)]
    lib.ntedit_hip_settle_info.argtypes = [vp, ctypes.POINTER(SettleStats)]
    # the reject filter (ntedit -e) from the same pass 2
    lib.ntedit_hip_filter_insert_solid2.argtypes = [vp, vp, u64, ci, u32, u32]
    lib.ntedit_hip_resident_insert_solid2.argtypes = [vp, u32, u32]
    lib.ntedit_hip_reads_set_reject_cutoff.argtypes = [vp, u32]
    # --gpu_parse on BGZF reads
    pmem = ctypes.POINTER(BgzfMember)
    lib.ntedit_hip_bgzf_walk.argtypes = [vp, u64, pmem, u64, pu64, pu64]
    lib.ntedit_hip_reads_inflate_device.argtypes = [vp, vp, u64, ci, pmem, u64, vp, u64, vp]
    lib.ntedit_hip_reads_inflate_model.argtypes = [vp, u64, pmem, u64, vp, u64, vp]
    lib.ntedit_hip_reads_last_record_start.argtypes = [vp, u64, ci]
    lib.ntedit_hip_reads_last_record_start.restype = u64
    lib.ntedit_hip_reads_last_start_device.argtypes = [vp, vp, u64, ci, pu64]
    lib.ntedit_hip_reads_inflate_info.argtypes = [vp, ctypes.POINTER(ReadsInflateStats)]
    # --gpu_parse on BAM reads
    bres = ctypes.POINTER(ReadsBamResult)
    lib.ntedit_hip_reads_is_bam.argtypes = [ctypes.c_char_p]
    lib.ntedit_hip_reads_bam_device.argtypes = [vp, vp, u64, ci, ci, u32, vp, u64, bres]
    lib.ntedit_hip_reads_bam_model.argtypes = [vp, u64, ci, u32, vp, u64, bres]
    lib.ntedit_hip_reads_bam_set_segment.argtypes = [vp, u64]
    lib.ntedit_hip_reads_bam_info.argtypes = [vp, ctypes.POINTER(ReadsBamStats)]
    # --gpu_parse for genome FASTA
    gres = ctypes.POINTER(GenomeParseResult)
    lib.ntedit_hip_genome_parse_device.argtypes = [vp, vp, u64, ci, ci, ci, vp, u64, gres]
    lib.ntedit_hip_genome_parse_model.argtypes = [vp, u64, ci, ci, vp, u64, gres]
    lib.ntedit_hip_genome_pass.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p), u32, u64, ci,
                                           ctypes.POINTER(ReadsPassStats)]
    lib.ntedit_hip_genome_pass_get_info.argtypes = [vp, ctypes.POINTER(GenomePassInfo)]
    lib.ntedit_hip_genome_pass_line.argtypes = [vp, ctypes.c_char_p, u64]
    # a store that outlives its sketch (ntedit --reads -k K1,K2,...)
    lib.ntedit_hip_sketch_reset.argtypes = [vp, u64, u32, u32]
    lib.ntedit_hip_resident_count.argtypes = [vp]
    lib.ntedit_hip_reads_set_min_read.argtypes = [vp, u32]
    # --min_qual: the context's setting, the last pass's counts, and the host-only calls with min_qual as one more argument
    lib.ntedit_hip_reads_set_min_qual.argtypes = [vp, u32]
    lib.ntedit_hip_reads_min_qual_info.argtypes = [vp, pu64, pu64]
    lib.ntedit_hip_reads_parse_model_q.argtypes = [vp, u64, u32, u32, vp, u64, pres]
    lib.ntedit_hip_reads_bam_model_q.argtypes = [vp, u64, ci, u32, u32, vp, u64, bres]
    lib.ntedit_hip_reads_range_text_q.argtypes = [ctypes.c_char_p, u64, u64, u32, vp, u64, pu64, pu64, pu64, pu64]
    # --min_read_len, --min_mean_qual, --min_rq: the context's setting, the last pass's counts, the host-only calls with the
    # filter as further arguments, and the lanes k_bam_facts gives a record
    pfs = ctypes.POINTER(ReadsReadFilterStats)
    lib.ntedit_hip_reads_set_read_filter.argtypes = [vp, u32, u32, ctypes.c_float]
    lib.ntedit_hip_reads_get_read_filter.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_float)]
    lib.ntedit_hip_reads_filter_options_check.argtypes = [ctypes.POINTER(ReadsFilterOptions), ci, ci, ctypes.POINTER(ReadsFilterRules)]
    lib.ntedit_hip_reads_read_filter_info.argtypes = [vp, pfs]
    lib.ntedit_hip_reads_parse_model_f.argtypes = [vp, u64, u32, u32, u32, u32, ctypes.c_float, vp, u64, pres, pfs]
    lib.ntedit_hip_reads_bam_model_f.argtypes = [vp, u64, ci, u32, u32, u32, u32, ctypes.c_float, vp, u64, bres, pfs]
    lib.ntedit_hip_reads_range_text_f.argtypes = [ctypes.c_char_p, u64, u64, u32, u32, u32, vp, u64, pu64, pu64, pu64, pu64, pfs]
    lib.ntedit_hip_reads_bam_set_group_width.argtypes = [vp, u32]
    lib.ntedit_hip_reads_bam_group_width.argtypes = [vp]
    # the edited draft in HBM and the k-mer QV (nte_apply.hip)
    pu32 = ctypes.POINTER(u32)
    lib.ntedit_hip_set_apply.argtypes = [vp, u32]
    lib.ntedit_hip_result_edited_device.argtypes = [vp, ctypes.POINTER(vp), pu64, vp, vp, u32]
    lib.ntedit_hip_result_edited.argtypes = [vp, vp, u64, pu64, vp, vp, u32]
    lib.ntedit_hip_result_last_error.argtypes = []
    lib.ntedit_hip_result_last_error.restype = ctypes.c_char_p
    lib.ntedit_hip_result_qv.argtypes = [vp, vp, u32]
    lib.ntedit_hip_qv_value.argtypes = [u64, u64, u32]
    lib.ntedit_hip_qv_value.restype = ctypes.c_double
    lib.ntedit_hip_qv_header.argtypes = []
    lib.ntedit_hip_qv_header.restype = ctypes.c_char_p
    lib.ntedit_hip_qv_format_row.argtypes = [ctypes.c_char_p, ctypes.POINTER(QvRow), u32, ctypes.c_char_p, u64]
    lib.ntedit_hip_apply_info.argtypes = [vp, ctypes.POINTER(ApplyStats)]
    lib.ntedit_hip_apply_tile.argtypes = []
    lib.ntedit_hip_apply_tile.restype = u32
    del pu32
    # the completeness marks (k_mark) and their estimator
    lib.ntedit_hip_shared_begin.argtypes = [vp]
    lib.ntedit_hip_shared_reset.argtypes = [vp]
    lib.ntedit_hip_shared_free.argtypes = [vp]
    lib.ntedit_hip_shared_free.restype = None
    lib.ntedit_hip_shared_mark.argtypes = [vp, ctypes.c_int, vp, u64, ctypes.c_int]
    lib.ntedit_hip_shared_download.argtypes = [vp, ctypes.c_int, vp]
    lib.ntedit_hip_shared_counts.argtypes = [vp, ctypes.POINTER(SharedStats)]
    lib.ntedit_hip_bloom_cardinality.argtypes = [u64, u64, u32]
    lib.ntedit_hip_bloom_cardinality.restype = ctypes.c_double
    lib.ntedit_hip_completeness_header.argtypes = []
    lib.ntedit_hip_completeness_header.restype = ctypes.c_char_p
    lib.ntedit_hip_completeness_format_row.argtypes = [ctypes.c_char_p, ctypes.POINTER(SharedStats), ctypes.c_int,
                                                       ctypes.c_char_p, u64]
    # the edited draft as BGZF (nte_bgzf_deflate.hip)
    pu32 = ctypes.POINTER(u32)
    lib.ntedit_hip_set_fa_names.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), u32]
    lib.ntedit_hip_result_fa_bgzf.argtypes = [vp, ctypes.POINTER(vp), pu64, pu64, pu32]
    lib.ntedit_hip_bgzf_deflate.argtypes = [vp, vp, u64, ci, vp, u64, pu64]
    lib.ntedit_hip_bgzf_deflate_model.argtypes = [vp, u64, vp, u64, pu64]
    lib.ntedit_hip_bgzf_bound.argtypes = [u64]
    lib.ntedit_hip_bgzf_bound.restype = u64
    lib.ntedit_hip_bgzf_eof.argtypes = [pu32]
    lib.ntedit_hip_bgzf_eof.restype = vp
    lib.ntedit_hip_bgzf_info.argtypes = [vp, ctypes.POINTER(BgzfStats)]
    # the unsupported regions as intervals (nte_track.hip)
    lib.ntedit_hip_result_track.argtypes = [vp, ci, vp, u64, pu64]
    lib.ntedit_hip_track_extract.argtypes = [vp, vp, u64, vp, vp, u32, u32, vp, u64, pu64]
    lib.ntedit_hip_track_info.argtypes = [vp, ctypes.POINTER(TrackStats)]
    lib.ntedit_hip_track_format_row.argtypes = [ctypes.c_char_p, ctypes.POINTER(TrackInterval), ctypes.c_char_p, u64]
    # the k-mer spectrum against a counting filter (k_spectrum)
    lib.ntedit_hip_set_spectrum.argtypes = [vp, ci]
    lib.ntedit_hip_result_spectrum.argtypes = [vp, ci, vp]
    lib.ntedit_hip_result_depth.argtypes = [vp, vp, u32]
    lib.ntedit_hip_spectrum_count.argtypes = [vp, vp, u64, ci, vp, vp, u32, vp, vp]
    lib.ntedit_hip_spectrum_info.argtypes = [vp, ctypes.POINTER(SpectrumStats)]
    lib.ntedit_hip_spectrum_header.restype = ctypes.c_char_p
    lib.ntedit_hip_spectrum_format_row.argtypes = [u32, u64, u64, ctypes.c_char_p, u64]
    lib.ntedit_hip_depth_header.restype = ctypes.c_char_p
    lib.ntedit_hip_depth_format_row.argtypes = [ctypes.c_char_p, ctypes.POINTER(DepthRow), ctypes.c_char_p, u64]
    # the spectrum by assembly copy number (nte_cn.hip)
    lib.ntedit_hip_set_cn.argtypes = [vp, ci, u64]
    lib.ntedit_hip_cn_append.argtypes = [vp, ci, vp, u64, ci, vp, vp, u32]
    lib.ntedit_hip_cn_finish.argtypes = [vp, u64]
    lib.ntedit_hip_cn_table.argtypes = [vp, ci, vp, vp]
    lib.ntedit_hip_cn_rows.argtypes = [vp, ci, vp, u64]
    lib.ntedit_hip_cn_distinct.argtypes = [vp, vp, vp]
    lib.ntedit_hip_cn_info.argtypes = [vp, ctypes.POINTER(CnStats)]
    lib.ntedit_hip_cn_reset.argtypes = [vp]
    lib.ntedit_hip_cn_free.argtypes = [vp]
    lib.ntedit_hip_cn_header.restype = ctypes.c_char_p
    lib.ntedit_hip_cn_format_row.argtypes = [u32, vp, vp, ctypes.c_char_p, u64]
    lib.ntedit_hip_cn_contig_header.restype = ctypes.c_char_p
    lib.ntedit_hip_cn_contig_format_row.argtypes = [ctypes.c_char_p, ctypes.POINTER(CnRow), ctypes.POINTER(CnRow), ctypes.c_char_p, u64]
    _lib = lib
    return lib
