"""ctypes binding of libmsim.so (include/msim.h) -- the only way the host package reaches the GPU.

There is no CPU fallback: if the library is missing or no MI355X is visible, ``Engine()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
LIB_CANDIDATES = [PKG_DIR.parent / "lib" / "libmsim.so"]

OK, ERR_ARG, ERR_HIP, ERR_VALUE, ERR_KEY, ERR_UNSUPPORTED, ERR_NOMEM, ERR_IO = range(8)
PLAN_AUTO, PLAN_HOST, PLAN_GPU = 0, 1, 2
RNG_FAST = 4           # Engine flag: counter-based generator, NOT stream-compatible with the reference (msim.h: MSIM_RNG_FAST)


class MsimError(RuntimeError):
    """A libmsim call failed (HIP error, bad argument, unsupported input).  ``code``: the MSIM_ERR_* value, where one came back."""
    code = None


class MsimUnsupported(MsimError):
    """Valid for the reference, outside this build's scope (translocations, >= 4 GiB contigs)."""


class Record(C.Structure):           # msim_record, 16 bytes
    _fields_ = [("pos", C.c_uint32), ("stop", C.c_uint32), ("extra", C.c_uint32),
                ("type", C.c_uint8), ("aux", C.c_uint8), ("rsv", C.c_uint16)]


RECORD_DTYPE = np.dtype([("pos", "<u4"), ("stop", "<u4"), ("extra", "<u4"), ("type", "u1"),
                         ("aux", "u1"), ("rsv", "<u2")])


class Range(C.Structure):            # msim_range
    _fields_ = [("start", C.c_int64), ("stop", C.c_int64), ("k", C.c_int64),
                ("setsize", C.c_int64), ("n_types", C.c_int32), ("types", C.c_int32 * 8),
                ("cdf_thr", C.c_uint64 * 8), ("min_len", C.c_int64 * 8), ("max_len", C.c_int64 * 8)]


class SettingsDesc(C.Structure):     # msim_settings_desc
    _fields_ = [("rate_sum", C.c_double), ("n_types", C.c_int32), ("types", C.c_int32 * 8), ("chances", C.c_double * 8),
                ("min_len", C.c_int64 * 8), ("max_len", C.c_int64 * 8)]


class Params(C.Structure):           # msim_params
    _fields_ = [("block", C.c_int64 * 8), ("ti_lim", C.c_uint64)]


class ReadsParams(C.Structure):      # msim_reads_params
    _fields_ = [("key", C.c_uint64), ("n_reads", C.c_uint64), ("len", C.c_uint32), ("paired", C.c_uint32),
                ("frag_min", C.c_uint32), ("n_frag", C.c_uint32), ("frag_thr", C.c_void_p), ("err_thr", C.c_void_p),
                ("qual", C.c_void_p), ("prefix", C.c_char_p)]


class PassItem(C.Structure):         # msim_pass_item
    _fields_ = [("contig", C.c_int32), ("flags", C.c_uint32), ("len", C.c_uint64), ("ranges", C.POINTER(Range)),
                ("n_ranges", C.c_int32), ("rsv", C.c_int32)]


PASS_APPLY = 1


class BatchContig(C.Structure):      # msim_batch_contig
    _fields_ = [("body", C.c_void_p), ("body_bytes", C.c_uint64), ("n_bases", C.c_uint64),
                ("lenc", C.c_uint32), ("lenb", C.c_uint32), ("ranges", C.POINTER(Range)),
                ("n_ranges", C.c_int32), ("name", C.c_char_p), ("header", C.c_char_p),
                ("name_len", C.c_uint32), ("header_len", C.c_uint32)]


# the same two structs as numpy record dtypes: a batch over an assembly builds its tables with array operations
RANGE_DTYPE = np.dtype([("start", "<i8"), ("stop", "<i8"), ("k", "<i8"), ("setsize", "<i8"), ("n_types", "<i4"),
                        ("types", "<i4", (8,)), ("_pad", "<i4"), ("cdf_thr", "<u8", (8,)), ("min_len", "<i8", (8,)),
                        ("max_len", "<i8", (8,))])
BATCH_CONTIG_DTYPE = np.dtype([("body", "<u8"), ("body_bytes", "<u8"), ("n_bases", "<u8"), ("lenc", "<u4"), ("lenb", "<u4"),
                               ("ranges", "<u8"), ("n_ranges", "<i4"), ("_pad", "<i4"), ("name", "<u8"), ("header", "<u8"),
                               ("name_len", "<u4"), ("header_len", "<u4")])


class Timing(C.Structure):           # msim_timing
    _fields_ = [("plan_host_ms", C.c_double), ("plan_gpu_ms", C.c_double),
                ("upload_ms", C.c_double), ("apply_ms", C.c_double),
                ("apply_kernel_ms", C.c_double), ("apply_launches", C.c_uint64),
                ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("records", C.c_uint64),
                ("py_words", C.c_uint64), ("np_words", C.c_uint64),
                ("contigs_snp", C.c_uint64), ("contigs_svmix", C.c_uint64), ("contigs_hostcut", C.c_uint64),
                ("contigs_hostchain", C.c_uint64), ("contigs_host", C.c_uint64), ("contigs_batch", C.c_uint64),
                ("contigs_fast", C.c_uint64), ("stream_rebases", C.c_uint64),
                ("snp_samples_ahead", C.c_uint64),
                ("host_walk_run_ms", C.c_double), ("host_walk_wait_ms", C.c_double),
                ("host_walk_candidates", C.c_uint64), ("host_cut_words", C.c_uint64),
                ("snp_ahead_margin_permille", C.c_uint64)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


# every symbol include/msim.h declares: (name, restype, argtypes)
_VP, _U8P, _U64P, _U32P, _IP = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), \
    C.POINTER(C.c_uint32), C.POINTER(C.c_int)
SYMBOLS = [
    ("msim_abi_version", C.c_int, []),
    ("msim_warm_up", C.c_int, [C.c_int]),
    ("msim_create", C.c_int, [C.c_int, C.c_uint32, C.POINTER(_VP)]),
    ("msim_destroy", None, [_VP]),
    ("msim_last_error", C.c_char_p, [_VP]),
    ("msim_device_name", C.c_int, [_VP, C.c_char_p, C.c_int]),
    ("msim_sync", C.c_int, [_VP]),
    ("msim_set_plan_mode", C.c_int, [_VP, C.c_uint32]),
    ("msim_seed", C.c_int, [_VP, _U32P, C.c_int, C.c_uint32]),
    ("msim_set_mt_state", C.c_int, [_VP, C.c_int, _U32P, C.c_int]),
    ("msim_get_mt_state", C.c_int, [_VP, C.c_int, _U32P, _IP]),
    ("msim_reserve_streams", C.c_int, [_VP, C.c_uint64, C.c_uint64]),
    ("msim_add_contig", C.c_int, [_VP, _VP, C.c_uint64, _IP]),
    ("msim_add_contig_synthetic", C.c_int, [_VP, C.c_uint64, C.c_uint64, _IP]),
    ("msim_contig_length", C.c_int, [_VP, C.c_int, _U64P]),
    ("msim_read_contig", C.c_int, [_VP, C.c_int, C.c_uint64, C.c_uint64, _VP]),
    ("msim_clear", C.c_int, [_VP]),
    ("msim_set_params", C.c_int, [_VP, C.POINTER(Params)]),
    ("msim_plan_contig", C.c_int, [_VP, C.c_int, C.POINTER(Range), C.c_int]),
    ("msim_plan_chain", C.c_int, [_VP, C.c_uint64, C.POINTER(Range), C.c_int]),
    ("msim_plan_pass", C.c_int, [_VP, C.POINTER(PassItem), C.c_int]),
    ("msim_dbg_pass_segments", C.c_int, [C.POINTER(Params), C.POINTER(PassItem), C.c_int, C.c_uint64, C.c_uint64, C.c_uint32,
                                         C.c_int, C.POINTER(C.c_int32)]),
    ("msim_plan_was_empty", C.c_int, [_VP, C.c_int, _IP]),
    ("msim_apply_contig", C.c_int, [_VP, C.c_int]),
    ("msim_key_error", C.c_int, [_VP, C.c_int, _U8P, _U64P]),
    ("msim_result_sizes", C.c_int, [_VP, C.c_int, _U64P, _U64P, _U64P]),
    ("msim_fetch_sequence", C.c_int, [_VP, C.c_int, C.c_uint64, C.c_uint64, _VP]),
    ("msim_fetch_records", C.c_int, [_VP, C.c_int, _VP, _VP]),
    ("msim_result_checksum", C.c_int, [_VP, C.c_int, _U64P]),
    ("msim_release_result", C.c_int, [_VP, C.c_int]),
    ("msim_result_device_ptr", C.c_int, [_VP, C.c_int, _U64P, _U64P]),
    ("msim_render_vcf", C.c_int, [_VP, C.c_uint64, _VP, _VP, C.c_uint64, C.c_char_p, _VP,
                                  C.c_uint64, _U64P]),
    ("msim_render_vcf_gt", C.c_int, [_VP, _VP, C.c_uint64, _VP, _VP, C.c_uint64, C.c_char_p, _VP, C.c_uint64, _U64P]),
    ("msim_genotype_contig", C.c_int, [_VP, C.c_int, C.c_uint64, C.c_uint32, C.c_uint64]),
    ("msim_set_genotypes", C.c_int, [_VP, C.c_int, _VP]),
    ("msim_fetch_genotypes", C.c_int, [_VP, C.c_int, _VP]),
    ("msim_select_haplotype", C.c_int, [_VP, C.c_int, C.c_int]),
    ("msim_render_chain", C.c_int, [_VP, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, _VP, C.c_uint64, _U64P]),
    ("msim_render_chain_device", C.c_int, [_VP, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64, _VP, C.c_uint64, _U64P]),
    ("msim_render_vcf_device", C.c_int, [_VP, C.c_int, C.c_char_p, _VP, C.c_uint64, _U64P]),
    ("msim_fetch_sequence_framed", C.c_int, [_VP, C.c_int, C.c_uint32, _VP, C.c_uint64, _U64P]),
    ("msim_render_vcf_device_file", C.c_int, [_VP, C.c_int, C.c_char_p, C.c_int, C.c_uint64, _U64P]),
    ("msim_fetch_sequence_framed_file", C.c_int, [_VP, C.c_int, C.c_uint32, C.c_int, C.c_uint64, _U64P]),
    ("msim_file_wait", C.c_int, [_VP]),
    ("msim_bgzf_open", C.c_int, [_VP, C.c_int, C.c_int]),
    ("msim_bgzf_append", C.c_int, [_VP, C.c_int, _VP, C.c_uint64]),
    ("msim_bgzf_close", C.c_int, [_VP, C.c_int, _U64P, _U64P]),
    ("msim_bgzf_bound", C.c_uint64, [C.c_uint64]),
    ("msim_bgzf_compress", C.c_int, [_VP, _VP, C.c_uint64, _VP, C.c_uint64, _U64P, C.POINTER(C.c_float)]),
    ("msim_bgzf_probe", C.c_int, [_VP, C.c_uint64, _U64P, _U64P]),
    ("msim_bgzf_inflate", C.c_int, [_VP, _VP, C.c_uint64, _VP, C.c_uint64, _U64P, C.POINTER(C.c_float)]),
    ("msim_vcf_load", C.c_int, [_VP, _VP, C.c_uint64, _U64P, _U64P]),
    ("msim_vcf_groups", C.c_int, [_VP, _VP, C.c_uint64, _U64P]),
    ("msim_vcf_select", C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("msim_vcf_plan_contig", C.c_int, [_VP, C.c_int, C.c_int64]),
    ("msim_vcf_host_bases", C.c_int, [_VP, C.c_int, _VP]),
    ("msim_vcf_timing", C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("msim_vcf_release", C.c_int, [_VP]),
    ("msim_device_host_cpus", C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    ("msim_batch_fetch_file", C.c_int, [_VP, C.c_int, C.c_uint64, C.c_int, C.c_uint64]),
    ("msim_add_contig_text", C.c_int, [_VP, _VP, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _IP]),
    ("msim_splice_contigs", C.c_int, [_VP, C.c_int, C.c_int, C.c_uint64, _U64P, _U64P, _IP]),
    ("msim_set_fast_key", C.c_int, [_VP, C.c_uint64]),
    ("msim_sample_min_distance", C.c_int, [_VP, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _VP]),
    ("msim_host_alloc", C.c_int, [_VP, C.c_uint64, C.POINTER(_VP)]),
    ("msim_host_free", C.c_int, [_VP, _VP]),
    ("msim_batch_run", C.c_int, [_VP, C.POINTER(BatchContig), C.c_int]),
    ("msim_batch_sizes", C.c_int, [_VP, C.c_int, _U64P, _U64P, C.POINTER(C.c_int32), _U64P]),
    ("msim_batch_fetch", C.c_int, [_VP, _VP, C.c_uint64, _VP, C.c_uint64]),
    ("msim_batch_view", C.c_int, [_VP, C.POINTER(C.c_void_p), _U64P, C.POINTER(C.c_void_p), _U64P, _U64P]),
    ("msim_batch_key_contig", C.c_int, [_VP, _IP]),
    ("msim_fasta_index", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _U64P]),
    ("msim_build_ranges", C.c_int, [_VP, C.c_int, _VP, _VP, _VP, C.c_int64, _VP]),
    ("msim_comm_unique_id", C.c_int, [_VP]),
    ("msim_comm_init", C.c_int, [_VP, _VP, C.c_int, C.c_int]),
    ("msim_comm_destroy", C.c_int, [_VP]),
    ("msim_planned_out_len", C.c_int, [_VP, C.c_int, _U64P, _IP]),
    ("msim_gather_to_root", C.c_int, [_VP, C.c_int, _IP, _IP, _U64P, _U64P, _U64P, C.c_int, _U64P]),
    ("msim_gather_plan", C.c_int, [C.c_int, _IP, _U64P, _U64P, _U64P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), _IP]),
    ("msim_gather_fetch", C.c_int, [_VP, C.c_uint64, C.c_uint64, _VP]),
    ("msim_dbg_snp_draws", C.c_int, [_VP, _VP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _VP, _VP, _U64P,
                                     _U32P, _VP]),
    ("msim_dbg_sample_tail", C.c_int, [_VP, _VP, C.c_uint64, _VP, C.c_uint64, C.c_uint32, _VP, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_uint32, _VP, C.c_uint32, _VP, C.c_int, C.c_uint64, C.c_uint32,
                                       C.c_uint32, C.c_uint64]),
    ("msim_dbg_chain_step", C.c_int, [_VP, _VP, C.c_uint64, _VP, _VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP, _VP, _VP]),
    ("msim_dbg_chains_fused", C.c_int, [_VP, _U64P]),
    ("msim_context_counts", C.c_int, [_VP, C.c_int, _VP, _U64P]),
    ("msim_plan_contig_spectrum", C.c_int, [_VP, C.c_int, _VP, C.c_uint64, C.c_uint32]),
    ("msim_spectrum_timing", C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("msim_dbg_context_counts", C.c_int, [_VP, C.c_uint64, _VP, _U64P]),
    ("msim_dbg_spectrum_plan", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, C.c_uint32, _VP, C.c_uint64, _U64P]),
    ("msim_sbs_counts", C.c_int, [_VP, C.c_int, _VP, _VP]),
    ("msim_sbs_timing", C.c_int, [_VP, C.POINTER(C.c_double)]),
    ("msim_dbg_sbs_counts", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP]),
    ("msim_cmp_hold", C.c_int, [_VP, C.c_int]),
    ("msim_cmp_release", C.c_int, [_VP, C.c_int]),
    ("msim_cmp_counts", C.c_int, [_VP, C.c_int, C.c_uint32, _VP, _VP]),
    ("msim_cmp_fetch", C.c_int, [_VP, C.c_int, _U64P, _U64P, _VP, _VP, _VP, _VP]),
    ("msim_cmp_timing", C.c_int, [_VP, C.POINTER(C.c_double)]),
    ("msim_dbg_cmp_counts", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64,
                                      C.c_uint32, _VP, _VP, _VP, _VP]),
    ("msim_cmp_counts_blocks", C.c_int, [_VP, C.c_int, C.c_uint32, C.c_uint32, _VP, _VP, _VP]),
    ("msim_cmp_blocks_timing", C.c_int, [_VP, C.POINTER(C.c_double)]),
    ("msim_dbg_cmp_counts_blocks", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64,
                                             C.c_uint32, C.c_uint32, _VP, _VP, _VP, _VP, _VP]),
    ("msim_cmp_join", C.c_int, [_VP, C.c_int, C.c_int]),
    ("msim_cmp_counts_diploid", C.c_int, [_VP, C.c_int, C.c_uint32, _VP, _VP]),
    ("msim_cmp_fetch_diploid", C.c_int, [_VP, C.c_int, C.c_int, _U64P, _U64P, _VP, _VP, _VP, _VP]),
    ("msim_cmp_join_timing", C.c_int, [_VP, C.POINTER(C.c_double)]),
    ("msim_cmp_phase_mark", C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _VP]),
    ("msim_cmp_phase_join", C.c_int, [_VP, C.c_int, C.c_int]),
    ("msim_cmp_phase_set", C.c_int, [_VP, C.c_int, C.c_int, _VP, C.c_uint64]),
    ("msim_cmp_phase_counts", C.c_int, [_VP, C.c_int, C.c_uint32, _VP]),
    ("msim_cmp_fetch_phase", C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP]),
    ("msim_cmp_phase_timing", C.c_int, [_VP, C.POINTER(C.c_double)]),
    ("msim_dbg_cmp_phase", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP, _VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP,
                                     C.c_uint32, _VP, _VP]),
    ("msim_dbg_vcf_phase_word", C.c_int, [_VP, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("msim_dbg_cmp_join", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP, _VP, _U64P]),
    ("msim_dbg_cmp_counts_diploid", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP, C.c_uint64, _VP,
                                              C.c_uint64, _VP, C.c_uint32, _VP, _VP, _VP, _VP]),
    ("msim_cmp_regions_set", C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP, C.c_uint64]),
    ("msim_cmp_regions_drop", C.c_int, [_VP, C.c_int, C.c_int]),
    ("msim_cmp_regions_mark", C.c_int, [_VP, C.c_int, C.c_uint32]),
    ("msim_cmp_counts_regions", C.c_int, [_VP, C.c_int, C.c_uint32, C.c_uint32, _VP, _VP]),
    ("msim_cmp_fetch_regions", C.c_int, [_VP, C.c_int, C.c_uint32, _VP, _VP]),
    ("msim_cmp_regions_timing", C.c_int, [_VP, C.POINTER(C.c_double)]),
    ("msim_dbg_cmp_counts_regions", C.c_int, [_VP, C.c_uint64, _VP, C.c_uint64, _VP, C.c_uint64, _VP, _VP, C.c_uint64, _VP, C.c_uint64, _VP,
                                              C.c_int, C.c_uint32, C.c_uint32, _VP, _VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP]),
    ("msim_bed_scan", C.c_int, [_VP, C.c_uint64, _VP, _VP, _VP, _U64P, _VP, _VP, _VP, _VP, _U64P]),
    ("msim_reads_setup", C.c_int, [_VP, C.POINTER(ReadsParams), _U64P, _U64P, _U64P]),
    ("msim_reads_render", C.c_int, [_VP, C.c_int, C.c_uint64, C.c_uint64, _VP, C.c_uint64]),
    ("msim_reads_render_file", C.c_int, [_VP, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _U64P]),
    ("msim_reads_timing", C.c_int, [_VP, C.POINTER(C.c_double), _VP]),
    ("msim_reads_release", C.c_int, [_VP]),
    ("msim_dbg_reads_render", C.c_int, [C.POINTER(ReadsParams), _VP, _VP, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, _VP, C.c_uint64,
                                        _U64P, _U64P, _U64P]),
    ("msim_stats", C.c_int, [_VP, C.POINTER(Timing)]),
    ("msim_reset_stats", C.c_int, [_VP]),
]
CMP_REGION_SETS = 8      # msim.h: MSIM_CMP_REGION_SETS, the region sets a contig keeps resident (a mark byte's bits)
CMP_DIPLOID = 2          # msim.h: MSIM_CMP_DIPLOID, the region calls' flag for the two diploid tables
CMP_EXACT = 1            # msim.h: MSIM_CMP_EXACT, the literal comparison
CMP_BINS = 5             # msim.h: MSIM_CMP_BINS, the length bins of IN and DE (1, 2-5, 6-20, 21-50, 51 and above)
CMP_PASS = 256           # msim.h: MSIM_CMP_PASS, the records one workgroup of the compare kernels takes per pass
CMP_WINDOW = 65536       # msim.h: MSIM_CMP_WINDOW, the bases an indel's placements stay inside
CMP_BLOCK_GAP = 50       # msim.h: MSIM_CMP_BLOCK_GAP, the default gap of compare --blocks (hap.py's superlocus window)
CMP_BLOCK_RECORDS, CMP_BLOCK_SPAN = 64, 4096     # msim.h: the records / the bases a block may hold and still be replayed
CMP_TRUTH, CMP_CALLS = 0, 1          # msim.h: MSIM_CMP_TRUTH, MSIM_CMP_CALLS, the sides of a diploid comparison
CMP_JOIN_TILE = 1024     # msim.h: MSIM_CMP_JOIN_TILE, the records one workgroup of the diploid join's scan takes
PHASE_CONTIG = 0xFFFFFFFF            # msim.h: MSIM_PHASE_CONTIG, the phase word of a record phased without a phase set
CMP_PHASE_TILE = 256     # msim.h: MSIM_CMP_PHASE_TILE, the records (and pairs) one workgroup of the phase passes takes
CMP_PHASE_COUNTS = 11    # msim.h: MSIM_CMP_PHASE_COUNTS, the values of msim_cmp_phase_counts
SPECTRUM_TILE = 4096     # msim.h: MSIM_SPECTRUM_TILE, the bases one workgroup of the spectrum sampler takes
SBS_CHANNELS, SBS_TALLIES = 96, 8    # msim.h: MSIM_SBS_CHANNELS, MSIM_SBS_TALLIES
SBS_PASS = 1024          # msim.h: MSIM_SBS_PASS, the records one workgroup of the profile kernel takes per pass

READS_MAX_LEN, READS_MAX_FRAG, READS_MAX_PREFIX = 512, 4096, 32      # msim.h: the limits of msim_reads_params

_lib = None


def library_path() -> Path:
    env = os.environ.get("MSIM_LIB")
    if env:
        return Path(env)
    for p in LIB_CANDIDATES:
        if p.exists():
            return p
    raise MsimError(
        f"libmsim.so not found (looked in {[str(p) for p in LIB_CANDIDATES]}); build it with "
        "`make -C mutation-simulator_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`")


def load():
    """dlopen libmsim.so and declare every prototype.  Never touches the GPU by itself."""
    global _lib
    if _lib is None:
        lib = C.CDLL(str(library_path()))
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.msim_abi_version() != 8:
            raise MsimError("libmsim ABI version mismatch")
        _lib = lib
    return _lib


def render_chain(recs: np.ndarray, length: int, t_name: str, q_name: str, chain_id: int) -> bytes:
    """``msim_render_chain``: the liftover chain of a record table (RECORD_DTYPE) over a contig of ``length`` bases.  Pure host
    code, no context."""
    lib = load()
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
    t, q = t_name.encode("utf-8", "replace"), q_name.encode("utf-8", "replace")
    need = C.c_uint64()
    rc = lib.msim_render_chain(_ptr(recs), len(recs), int(length), t, q, int(chain_id), None, 0, C.byref(need))
    if rc != OK:
        raise MsimError(f"msim_render_chain failed ({rc})")
    out = np.empty(need.value, dtype=np.uint8)
    if need.value:
        rc = lib.msim_render_chain(_ptr(recs), len(recs), int(length), t, q, int(chain_id), _ptr(out), need.value, C.byref(need))
        if rc != OK:
            raise MsimError(f"msim_render_chain failed ({rc})")
    return out.tobytes()


# the device tables of the SV-mix / host-chain test hooks (csrc/plan_kernels.h: TypeTable, MixRangeDev)
TYPE_TABLE_DTYPE = np.dtype([("thr", "<u8", (8,)), ("n", "<u4"), ("type", "u1", (8,)), ("_pad", "u1", (4,))])
MIX_RANGE_DTYPE = np.dtype([("rec_base", "<u4"), ("clip", "<u4"), ("set_id", "<u4"), ("rsv", "<u4")])
TAIL_STATE_DTYPE = np.dtype([("pos", "<u8"), ("snp_base", "<u8"), ("flags", "<u4"), ("dups", "<u4"), ("accepted_used", "<u4"),
                             ("rsv", "<u4")])      # msim_dbg_tail_state
CHAIN_STEP_DTYPE = np.dtype([("lo", "<u8"), ("expect", "<u8"), ("pos_limit", "<u8"), ("snp_limit", "<u8"), ("ti_lim", "<u8")] +
                            [(f, "<u4") for f in ("F", "K", "k_core", "shift", "n", "W", "W2", "K2", "soft_half", "G", "core_dups",
                                                  "core_flags", "head_flags", "bm_guard", "fused", "rsv")] +
                            [("state", TAIL_STATE_DTYPE), ("hdr", "<u4", (4,)), ("base", "<u8")])      # msim_dbg_chain
CHAIN_DROPPED = 0xFFFFFFFF           # ctx.h: a chain candidate that is blocked / dropped
CHAIN_TOMBSTONE = 0x80               # ctx.h: ch_aux flag of an entry __fix_tl_amount deleted


def chain_lg_rows(n_classes: int) -> int:
    """log2 of the accept tables' slots per word position (ctx.h: chain_lg_rows)."""
    return 0 if n_classes <= 1 else 1 if n_classes == 2 else 2 if n_classes <= 4 else 3


def accept_tables_host(tempered, classes) -> np.ndarray:
    """The host's accept tables (plan_host.cpp: accept_tables_host) over TEMPERED words for ``classes`` = [(shift, width)], shape
    (len(tempered) + 1, 1 << lg_rows).  Pure host code, no context (msim_dbg_accept_tables_host: not part of include/msim.h)."""
    fn = load().msim_dbg_accept_tables_host
    fn.restype, fn.argtypes = C.c_int, [_VP, C.c_uint32, _VP, _VP, C.c_uint32, _VP]
    words = np.ascontiguousarray(tempered, dtype=np.uint32)
    sh = np.array([c[0] for c in classes], dtype=np.uint32)
    width = np.array([c[1] for c in classes], dtype=np.uint32)
    T = np.full((len(words) + 1, 1 << chain_lg_rows(len(classes))), 0xdddddddd, dtype=np.uint32)
    rc = fn(_ptr(words), len(words), _ptr(sh), _ptr(width), len(classes), _ptr(T))
    if rc != OK:
        err = MsimError(f"msim_dbg_accept_tables_host failed ({rc})")
        err.code = rc
        raise err
    return T


def chain_tile() -> int:
    """Records / gaps a workgroup of the chain kernels takes (text_gpu.hip: CH_TILE): where the device renderer's edge cases
    lie (msim_dbg_chain_tile: exported, not part of include/msim.h)."""
    fn = load().msim_dbg_chain_tile
    fn.restype, fn.argtypes = C.c_uint32, []
    return int(fn())


def reads_group(stride: int) -> int:
    """Reads a workgroup of the render kernel takes at this record stride (reads.hip: reads_per_group): where the edge cases of
    a chunk split lie (msim_dbg_reads_group: exported, not part of include/msim.h)."""
    fn = load().msim_dbg_reads_group
    fn.restype, fn.argtypes = C.c_uint32, [C.c_uint32]
    return int(fn(int(stride)))


def parse_cpulist(text: str) -> set:
    """A Linux cpulist ("0-63,128-191") as a set of ints."""
    out = set()
    for part in text.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        out.update(range(int(a), int(b or a) + 1))
    return out


def warm_up_async(device: int = 0, pin: bool = False):
    """Start the HIP runtime on a helper thread (the first HIP call of a process costs ~0.2 s) while the caller reads and
    indexes its input; returns the thread (join it, or just create the Engine: HIP initialisation is serialised inside).
    ``pin``: once the runtime is up, move the CALLING thread onto the CPUs of the GPU's NUMA node (what the CLI does:
    on a two-socket host the copies to and from the GPU then cross the inter-socket links once; ``MSIM_NO_PIN=1`` or a
    cpuset that does not contain those CPUs leaves it where it is)."""
    import threading
    lib = load()
    caller = threading.get_native_id()

    def work():
        lib.msim_warm_up(int(device))
        if not pin or os.environ.get("MSIM_NO_PIN") == "1" or not hasattr(os, "sched_setaffinity"):
            return
        try:
            buf = C.create_string_buffer(4096)
            if lib.msim_device_host_cpus(int(device), buf, 4096) != OK or not buf.value:
                return
            cpus = parse_cpulist(buf.value.decode()) & os.sched_getaffinity(caller)
            if cpus:
                os.sched_setaffinity(caller, cpus)
        except (OSError, ValueError):
            pass
    t = threading.Thread(target=work, name="msim-warm-up", daemon=True)
    t.start()
    return t


def _ptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data)


def reads_params(key: int, n_reads: int, length: int, paired: bool, frag_min: int, frag_thr, err_thr, qual, prefix: str):
    """``msim_reads_params`` over the caller's tables: (the struct, the arrays it points into -- keep them while it is used)."""
    frag_thr = np.ascontiguousarray(frag_thr, dtype=np.uint64).reshape(-1)
    err_thr = np.ascontiguousarray(err_thr, dtype=np.uint64).reshape(-1)
    qual = np.ascontiguousarray(qual, dtype=np.uint8).reshape(-1)
    if err_thr.shape[0] != 2 * int(length) or qual.shape[0] != 2 * int(length):
        raise MsimError("reads: err_thr and qual hold 2 x LEN entries")
    p = ReadsParams()
    p.key, p.n_reads, p.len, p.paired = int(key) & (2**64 - 1), int(n_reads), int(length), 1 if paired else 0
    p.frag_min, p.n_frag = int(frag_min), int(frag_thr.shape[0])
    p.frag_thr, p.err_thr, p.qual = frag_thr.ctypes.data, err_thr.ctypes.data, qual.ctypes.data
    p.prefix = prefix.encode("utf-8", "replace")
    return p, (frag_thr, err_thr, qual)


def dbg_reads_render(params, contigs, mate: int, first: int, count: int):
    """``msim_dbg_reads_render``: records [first, first + count) of ``mate`` by the library's sequential host loop over
    ``contigs`` (a list of uint8 arrays, upper case): (text as bytes, stride, eligible contigs, P).  No context, no GPU."""
    lib = load()
    p, keep = params
    offsets = np.zeros(len(contigs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in contigs], dtype=np.uint64)
    bases = np.concatenate([np.asarray(x, dtype=np.uint8) for x in contigs]) if contigs else np.zeros(0, np.uint8)
    bases = np.ascontiguousarray(bases)
    stride, n_elig, P = C.c_uint64(), C.c_uint64(), C.c_uint64()

    def call(out, cap):
        rc = lib.msim_dbg_reads_render(C.byref(p), _ptr(bases), _ptr(offsets), len(contigs), int(mate), int(first), int(count), out, cap,
                                       C.byref(stride), C.byref(n_elig), C.byref(P))
        if rc != OK:
            msg = lib.msim_last_error(None).decode()
            err = ValueError(msg) if rc == ERR_VALUE else MsimUnsupported(msg) if rc == ERR_UNSUPPORTED else MsimError(f"libmsim error {rc}: {msg}")
            if not isinstance(err, ValueError):
                err.code = rc
            raise err
    call(None, 0)
    out = np.empty(int(count) * stride.value, dtype=np.uint8)
    if count:
        call(_ptr(out), out.shape[0])
    del keep
    return out.tobytes(), stride.value, n_elig.value, P.value


class Engine:
    """One libmsim context (one GPU).  Thin, typed wrappers -- no logic lives here."""

    def __init__(self, device: int = 0, flags: int = PLAN_AUTO):
        self.lib = load()
        self.h = C.c_void_p()
        if flags == PLAN_AUTO and os.environ.get("MSIM_PLAN_MODE"):      # diagnosis: 1 = host planner everywhere, 2 = device engines only
            flags = int(os.environ["MSIM_PLAN_MODE"])
        rc = self.lib.msim_create(device, flags, C.byref(self.h))
        if rc != OK:
            msg = self.lib.msim_last_error(None).decode()
            self.h = None
            raise MsimError(f"msim_create failed ({rc}): {msg}")
        self._pinned: list = []

    def close(self):
        if getattr(self, "h", None):
            for p in getattr(self, "_pinned", []):
                self.lib.msim_host_free(self.h, C.c_void_p(p))
            self._pinned = []
            self.lib.msim_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ errors
    def _check(self, rc: int, contig: int | None = None):
        if rc == OK:
            return
        msg = self.lib.msim_last_error(self.h).decode()
        if rc == ERR_VALUE:
            raise ValueError(msg)                      # the reference's own exception (util.py:104)
        if rc == ERR_KEY:
            base = C.c_uint8()
            pos = C.c_uint64()
            self.lib.msim_key_error(self.h, -1, C.byref(base),
                                    C.byref(pos))
            raise KeyError(chr(base.value))            # mutator.py:449-455
        err = MsimUnsupported(msg) if rc == ERR_UNSUPPORTED else MsimError(f"libmsim error {rc}: {msg}")
        err.code = rc
        raise err

    # ------------------------------------------------------------------ device / rng
    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self.lib.msim_device_name(self.h, buf, 256))
        return buf.value.decode()

    def sync(self):
        self._check(self.lib.msim_sync(self.h))

    def seed(self, py_seed: int, np_seed: int):
        n = abs(int(py_seed))
        key = []
        while True:
            key.append(n & 0xFFFFFFFF)
            n >>= 32
            if not n:
                break
        arr = (C.c_uint32 * len(key))(*key)
        self._check(self.lib.msim_seed(self.h, arr, len(key), int(np_seed) & 0xFFFFFFFF))

    def set_mt_state(self, stream: int, mt, pos: int):
        arr = np.ascontiguousarray(mt, dtype=np.uint32)
        assert arr.shape == (624,)
        self._check(self.lib.msim_set_mt_state(self.h, stream, arr.ctypes.data_as(_U32P), int(pos)))

    def get_mt_state(self, stream: int):
        arr = np.zeros(624, dtype=np.uint32)
        pos = C.c_int()
        self._check(self.lib.msim_get_mt_state(self.h, stream, arr.ctypes.data_as(_U32P),
                                               C.byref(pos)))
        return arr, pos.value

    def set_fast_key(self, key: int):
        """Key of the counter-based generator of a ``RNG_FAST`` context (restarts its contig ordinal)."""
        self._check(self.lib.msim_set_fast_key(self.h, int(key) & 0xFFFFFFFFFFFFFFFF))

    def reserve_streams(self, py_words: int, np_words: int = 0):
        self._check(self.lib.msim_reserve_streams(self.h, int(py_words), int(np_words)))

    # ------------------------------------------------------------------ genome
    def add_contig(self, bases: np.ndarray) -> int:
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        cid = C.c_int()
        self._check(self.lib.msim_add_contig(self.h, _ptr(bases), bases.shape[0], C.byref(cid)))
        return cid.value

    def add_contig_text(self, body: np.ndarray, n_bases: int, lenc: int, lenb: int) -> int:
        """One FASTA record straight from file text (bytes after the header line); the device skips the
        line terminators and upper-cases."""
        body = np.ascontiguousarray(body, dtype=np.uint8)
        cid = C.c_int()
        self._check(self.lib.msim_add_contig_text(self.h, _ptr(body), body.shape[0], n_bases, lenc, lenb, C.byref(cid)))
        return cid.value

    def sample_min_distance(self, start: int, stop: int, k: int, d: int, setsize: int) -> np.ndarray:
        """``sample_with_minimum_distance`` (util.py:93-109) on this context's CPython stream; ValueError as CPython's."""
        out = np.empty(max(int(k), 0), dtype=np.int64)
        self._check(self.lib.msim_sample_min_distance(self.h, int(start), int(stop), int(k), int(d), int(setsize),
                                                      C.c_void_p(out.ctypes.data)))
        return out

    def splice_contigs(self, a: int, b: int, bp_a, bp_b) -> int:
        """Interchromosomal translocation of contig ``a`` with partner ``b`` (it_mutator.py:121-146): a new contig made of
        a's and b's segments between the breakpoints, taken alternately.  No breakpoints: a copy of ``a``."""
        bp_a = np.ascontiguousarray(bp_a, dtype=np.uint64)
        bp_b = np.ascontiguousarray(bp_b, dtype=np.uint64)
        if bp_a.shape != bp_b.shape or bp_a.ndim != 1:
            raise ValueError("both contigs need the same number of breakpoints")
        cid = C.c_int()
        n = int(bp_a.shape[0])
        self._check(self.lib.msim_splice_contigs(self.h, a, b, n, C.cast(C.c_void_p(bp_a.ctypes.data), _U64P) if n else None,
                                                 C.cast(C.c_void_p(bp_b.ctypes.data), _U64P) if n else None, C.byref(cid)))
        return cid.value

    def host_buffer(self, nbytes: int) -> np.ndarray:
        """A page-locked uint8 buffer owned by this engine (freed at ``close``): ingest / egress through it runs at the
        link's speed (no staging pass, no page faults of a fresh allocation)."""
        p = _VP()
        self._check(self.lib.msim_host_alloc(self.h, int(nbytes), C.byref(p)))
        self._pinned.append(p.value)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(int(nbytes), 1),))[:nbytes]

    def add_contig_synthetic(self, length: int, seed: int) -> int:
        cid = C.c_int()
        self._check(self.lib.msim_add_contig_synthetic(self.h, length, seed, C.byref(cid)))
        return cid.value

    def contig_length(self, contig: int) -> int:
        n = C.c_uint64()
        self._check(self.lib.msim_contig_length(self.h, contig, C.byref(n)))
        return n.value

    def read_contig(self, contig: int, offset: int = 0, n: int | None = None) -> np.ndarray:
        if n is None:
            n = self.contig_length(contig) - offset
        out = np.empty(n, dtype=np.uint8)
        self._check(self.lib.msim_read_contig(self.h, contig, offset, n, _ptr(out)))
        return out

    def clear(self):
        self._check(self.lib.msim_clear(self.h))

    # ------------------------------------------------------------------ plan / apply
    def set_params(self, params: Params):
        self._check(self.lib.msim_set_params(self.h, C.byref(params)))

    @staticmethod
    def range_table(ranges: list):
        """The ctypes array `plan_contig` passes on; a caller that plans the same contig repeatedly may build it once."""
        arr = (Range * max(len(ranges), 1))(*ranges)
        arr.n_ranges = len(ranges)
        return arr

    @staticmethod
    def _ranges_arg(ranges):
        """(pointer, count, keep-alive) of a range table given as a list of ``Range``, a ctypes array or a numpy
        ``RANGE_DTYPE`` table (``mutator.plan_table``)."""
        if isinstance(ranges, np.ndarray):
            if ranges.dtype != RANGE_DTYPE:
                raise MsimError("range table of the wrong dtype")
            ranges = np.ascontiguousarray(ranges)
            return C.cast(C.c_void_p(ranges.ctypes.data), C.POINTER(Range)), int(ranges.shape[0]), ranges
        arr = ranges if isinstance(ranges, C.Array) else Engine.range_table(ranges)
        return arr, getattr(arr, "n_ranges", len(arr)), arr

    def plan_contig(self, contig: int, ranges):
        ptr, n, keep = self._ranges_arg(ranges)
        self._check(self.lib.msim_plan_contig(self.h, contig, ptr, n), contig)
        del keep

    def plan_chain(self, length: int, ranges):
        """Advance both streams over a contig this process does not mutate (multi-GPU: a rank that does not own it)."""
        ptr, n, keep = self._ranges_arg(ranges)
        self._check(self.lib.msim_plan_chain(self.h, length, ptr, n))
        del keep

    @staticmethod
    def pass_items(items):
        """The ctypes table ``plan_pass`` hands on, from ``(contig, ranges, apply)`` triples in pass order -- ``contig`` a libmsim
        id, or ``None`` with ``length`` given as a fourth element for a contig that is only walked (``msim_plan_chain``).  Returns
        (table, keep-alive)."""
        arr = (PassItem * max(len(items), 1))()
        keep = []
        for slot, it in zip(arr, items):
            contig, ranges, apply = it[0], it[1], it[2]
            ptr, n, k = Engine._ranges_arg(ranges)
            keep.append(k)
            slot.contig = -1 if contig is None else int(contig)
            slot.flags = PASS_APPLY if (apply and contig is not None) else 0
            slot.len = int(it[3]) if contig is None else 0
            slot.ranges = C.cast(ptr, C.POINTER(Range))
            slot.n_ranges = n
        return arr, keep

    def plan_pass(self, items):
        """A whole pass in one call (``msim_plan_pass``): item by item what ``plan_contig`` / ``plan_chain`` / ``apply_contig``
        would do in the same order, with the SNP sampler's off-chain work of the contigs to come enqueued up front."""
        arr, keep = self.pass_items(items)
        self._check(self.lib.msim_plan_pass(self.h, arr, len(items)))
        del keep

    def set_plan_mode(self, mode: int):
        """0 = AUTO, PLAN_HOST = force the sequential host planner, PLAN_GPU = force a device engine."""
        self._check(self.lib.msim_set_plan_mode(self.h, mode))

    def plan_was_empty(self, contig: int) -> bool:
        e = C.c_int()
        self._check(self.lib.msim_plan_was_empty(self.h, contig, C.byref(e)))
        return bool(e.value)

    def apply_contig(self, contig: int):
        self._check(self.lib.msim_apply_contig(self.h, contig), contig)

    def result_sizes(self, contig: int, applied: bool = True):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_result_sizes(self.h, contig, C.byref(a) if applied else None,
                                               C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def fetch_sequence(self, contig: int, offset: int = 0, n: int | None = None) -> np.ndarray:
        if n is None:
            n = self.result_sizes(contig)[0] - offset
        out = np.empty(n, dtype=np.uint8)
        self._check(self.lib.msim_fetch_sequence(self.h, contig, offset, n, _ptr(out)))
        return out

    def fetch_records(self, contig: int):
        _, n_rec, n_pool = self.result_sizes(contig, applied=False)
        recs = np.zeros(n_rec, dtype=RECORD_DTYPE)
        pool = np.zeros(n_pool, dtype=np.uint8)
        self._check(self.lib.msim_fetch_records(self.h, contig, _ptr(recs), _ptr(pool)))
        return recs, pool

    # ------------------------------------------------------------------ diploid runs (msim.h: genotypes, haplotype selection)
    def genotype_contig(self, contig: int, key: int, seq: int, het_thr: int):
        """Draw a genotype byte (1: haplotype 1, 2: haplotype 2, 3: both) for every record of the planned contig's table:
        Philox counter (record index, 0, ``seq``, tag 20) under the 64-bit ``key``; heterozygous iff the 53-bit sample is below
        ``het_thr`` = ceil(F * 2**53).  No MT19937 stream moves."""
        self._check(self.lib.msim_genotype_contig(self.h, contig, int(key) & (2**64 - 1), int(seq), int(het_thr)), contig)

    def set_genotypes(self, contig: int, gt: np.ndarray):
        gt = np.ascontiguousarray(gt, dtype=np.uint8)
        self._check(self.lib.msim_set_genotypes(self.h, contig, _ptr(gt)), contig)

    def fetch_genotypes(self, contig: int, n_records: int) -> np.ndarray:
        """The genotype bytes of the contig's FULL table (``n_records``: its size, whichever haplotype is selected)."""
        out = np.zeros(n_records, dtype=np.uint8)
        self._check(self.lib.msim_fetch_genotypes(self.h, contig, _ptr(out)), contig)
        return out

    def select_haplotype(self, contig: int, hap: int):
        """``hap`` 1 / 2: the records on that haplotype become the contig's active table (APPLY, sizes, record fetch, chain);
        0: the full table again.  The VCF text is always the full table's."""
        self._check(self.lib.msim_select_haplotype(self.h, contig, int(hap)), contig)

    # ------------------------------------------------------------------ VCF replay (msim.h: msim_vcf_*)
    def vcf_load(self, text) -> tuple:
        """The whole VCF text (bytes-like / uint8 array) into the context, parsed into lines and groups once; returns
        (lines, groups).  The caller's buffer is free again when this returns."""
        buf = _as_u8(text)
        n = int(buf.shape[0])
        lines, groups = C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_vcf_load(self.h, C.c_void_p(buf.ctypes.data) if n else None, n, C.byref(lines), C.byref(groups)))
        return lines.value, groups.value

    def vcf_groups(self) -> np.ndarray:
        """The runs of data lines with one CHROM, in file order (``VCF_GROUP_DTYPE``)."""
        n = C.c_uint64()
        self._check(self.lib.msim_vcf_groups(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=VCF_GROUP_DTYPE)
        if n.value:
            self._check(self.lib.msim_vcf_groups(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def vcf_select(self, grammar: int, sample_index: int = 0, haplotype: int = 1):
        """The grammar the following ``vcf_plan_contig`` calls read with: 0 the simulator's dialect, 1 consensus (any VCF; the
        0-based sample column and the 1-based haplotype to follow).  ``vcf_load`` selects 0 again."""
        self._check(self.lib.msim_vcf_select(self.h, int(grammar), int(sample_index), int(haplotype)))

    def vcf_plan_contig(self, contig: int, group: int = -1):
        """Group ``group`` (-1: no lines) becomes the contig's record table and insert pool, validated against its bases;
        ``ValueError`` ("VCF line N: reason") for a line the rewrite is not written for.  ``apply_contig`` follows."""
        self._check(self.lib.msim_vcf_plan_contig(self.h, int(contig), int(group)), contig)

    def vcf_host_bases(self, contig: int, bases: np.ndarray):
        """Host-only contexts keep no bases: the contig's (upper-cased, its whole length) for the host parser.  A no-op on a
        device context."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        assert bases.shape[0] == self.contig_length(contig)
        self._check(self.lib.msim_vcf_host_bases(self.h, int(contig), _ptr(bases)), contig)

    def vcf_timing(self) -> tuple:
        """(load, plan) kernel milliseconds since ``vcf_load`` (HIP events)."""
        a, b = C.c_double(), C.c_double()
        self._check(self.lib.msim_vcf_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def vcf_release(self):
        self._check(self.lib.msim_vcf_release(self.h))

    # ------------------------------------------------------------------ context-dependent SNPs (msim.h: a 96-channel spectrum)
    def context_counts(self, contig: int):
        """Device census of a resident contig: (counts of its eligible sites per trinucleotide context, uint64[64]; their sum)."""
        counts = np.zeros(64, dtype=np.uint64)
        n = C.c_uint64()
        self._check(self.lib.msim_context_counts(self.h, int(contig), _ptr(counts), C.byref(n)), contig)
        return counts, n.value

    def plan_contig_spectrum(self, contig: int, thr, key: int, seq: int):
        """Every eligible site of the contig mutates by its own Philox draw (counter (site >> 1, 0, ``seq``, tag 21) under the
        64-bit ``key``) against ``thr`` (192 thresholds, ``spectrum.thresholds``); leaves the contig planned."""
        thr = _thr_array(thr)
        self._check(self.lib.msim_plan_contig_spectrum(self.h, int(contig), _ptr(thr), int(key) & (2**64 - 1), int(seq)), contig)

    def spectrum_timing(self) -> tuple:
        """(census, plan) kernel milliseconds since ``reset_stats`` (HIP events)."""
        a, b = C.c_double(), C.c_double()
        self._check(self.lib.msim_spectrum_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sbs_counts(self, contig: int) -> tuple:
        """The SBS-96 profile of a planned contig's record table against its resident reference bases: (SN records per channel
        in ``spectrum.CHANNELS`` order, uint64[96]; tallies, uint64[8]: [0] SN records without a channel, [t] records of type t)."""
        channels = np.zeros(SBS_CHANNELS, dtype=np.uint64)
        tallies = np.zeros(SBS_TALLIES, dtype=np.uint64)
        self._check(self.lib.msim_sbs_counts(self.h, int(contig), _ptr(channels), _ptr(tallies)), contig)
        return channels, tallies

    def sbs_timing(self) -> float:
        """The profile kernel's milliseconds since ``reset_stats`` (HIP events)."""
        a = C.c_double()
        self._check(self.lib.msim_sbs_timing(self.h, C.byref(a)))
        return a.value

    # ------------------------------------------------------------------ reads (msim.h: FASTQ records from the resident genome)
    def reads_setup(self, params) -> tuple:
        """Check and upload the tables of a reads run (``reads_params``) over the context's contigs: (stride, eligible
        contigs, P)."""
        p, _keep = params
        stride, n_elig, P = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_reads_setup(self.h, C.byref(p), C.byref(stride), C.byref(n_elig), C.byref(P)))
        self._reads_stride = stride.value
        return stride.value, n_elig.value, P.value

    def reads_render(self, mate: int, first: int, count: int) -> bytes:
        """Records [first, first + count) of mate 0 / 1 as bytes."""
        out = np.empty(int(count) * self._reads_stride, dtype=np.uint8)
        self._check(self.lib.msim_reads_render(self.h, int(mate), int(first), int(count), _ptr(out), out.shape[0]))
        return out.tobytes()

    def reads_render_to_file(self, mate: int, first: int, count: int, fd: int, offset: int) -> int:
        """The same records queued for bytes [offset, ...) of ``fd`` on output channel ``mate``; returns their byte count."""
        n = C.c_uint64()
        self._check(self.lib.msim_reads_render_file(self.h, int(mate), int(first), int(count), int(fd), int(offset), C.byref(n)))
        return n.value

    def reads_timing(self) -> tuple:
        """(render kernel milliseconds since ``reset_stats``, reads of mate 1 / mate 2 that hold only N since the last setup)."""
        ms = C.c_double()
        all_n = np.zeros(2, dtype=np.uint64)
        self._check(self.lib.msim_reads_timing(self.h, C.byref(ms), _ptr(all_n)))
        return ms.value, (int(all_n[0]), int(all_n[1]))

    def reads_release(self):
        self._check(self.lib.msim_reads_release(self.h))

    # ------------------------------------------------------------------ compare (msim.h: a truth table against a calls table)
    def cmp_hold(self, contig: int):
        """A device copy of the planned contig's current table (records and insert pool) becomes its held table: the truth
        of the following ``cmp_counts``.  It survives a new plan of the contig and ``release_result``."""
        self._check(self.lib.msim_cmp_hold(self.h, int(contig)), contig)

    def cmp_release(self, contig: int = -1):
        """Drop the contig's held table (-1: every contig's)."""
        self._check(self.lib.msim_cmp_release(self.h, int(contig)))

    def _cmp_counts(self, fn, width: int, contig: int, exact: bool) -> tuple:
        counts = np.zeros((8, CMP_BINS, width), dtype=np.uint64)
        tallies = np.zeros(2, dtype=np.uint64)
        self._check(fn(self.h, int(contig), CMP_EXACT if exact else 0, _ptr(counts), _ptr(tallies)), contig)
        return counts, tallies

    def cmp_counts(self, contig: int, exact: bool = False) -> tuple:
        """The contig's held table (truth) scored against its current one (calls): (uint64[8, CMP_BINS, 4] by record type and
        length bin -- truth matched, truth missed, calls matched, calls extra; uint64[2]: truth indels whose walk a window edge
        stopped, ... a byte outside ACGT stopped).  ``exact``: the literal comparison, no shifting."""
        return self._cmp_counts(self.lib.msim_cmp_counts, 4, contig, exact)

    def cmp_fetch(self, contig: int, flags: bool = True) -> tuple:
        """(held records, held pool, a flag byte per held record, a flag byte per current record) of the contig's last
        ``cmp_counts``; 1 = matched.  ``flags=False``: the held table only (the flag arrays are None)."""
        n, m = C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_cmp_fetch(self.h, int(contig), C.byref(n), C.byref(m), None, None, None, None), contig)
        recs = np.zeros(n.value, dtype=RECORD_DTYPE)
        pool = np.zeros(m.value, dtype=np.uint8)
        fa = fb = None
        if flags:
            fa = np.zeros(n.value, dtype=np.uint8)
            fb = np.zeros(self.result_sizes(contig, applied=False)[1], dtype=np.uint8)
        self._check(self.lib.msim_cmp_fetch(self.h, int(contig), None, None, _ptr(recs), _ptr(pool),
                                            _ptr(fa) if flags else None, _ptr(fb) if flags else None), contig)
        return recs, pool, fa, fb

    def cmp_timing(self) -> float:
        """The compare kernels' milliseconds since ``reset_stats`` (HIP events)."""
        a = C.c_double()
        self._check(self.lib.msim_cmp_timing(self.h, C.byref(a)))
        return a.value

    def cmp_counts_blocks(self, contig: int, exact: bool = False, gap: int = CMP_BLOCK_GAP) -> tuple:
        """``cmp_counts`` with the unmatched records rescued block by block (msim.h: compare --blocks): (uint64[8, CMP_BINS, 6] --
        truth matched, truth block-matched, truth missed, calls matched, calls block-matched, calls extra; uint64[2] as
        ``cmp_counts``; uint64[5]: candidates, replayed, equal, over a limit, holding a translocation).  ``cmp_fetch`` then
        gives flag bytes 0, 1 or 2 (matched as part of a block)."""
        counts = np.zeros((8, CMP_BINS, 6), dtype=np.uint64)
        tallies = np.zeros(2, dtype=np.uint64)
        blocks = np.zeros(5, dtype=np.uint64)
        self._check(self.lib.msim_cmp_counts_blocks(self.h, int(contig), CMP_EXACT if exact else 0, int(gap), _ptr(counts),
                                                    _ptr(tallies), _ptr(blocks)), contig)
        return counts, tallies, blocks

    def cmp_blocks_timing(self) -> float:
        """The block pass's milliseconds on the device since ``reset_stats`` (HIP events)."""
        a = C.c_double()
        self._check(self.lib.msim_cmp_blocks_timing(self.h, C.byref(a)))
        return a.value

    def cmp_join(self, contig: int, side: int):
        """The contig's held table (haplotype 1) and its current table (haplotype 2) joined into its diploid table of ``side``
        (``CMP_TRUTH`` / ``CMP_CALLS``): distinct variants with a genotype byte each.  The held table is consumed."""
        self._check(self.lib.msim_cmp_join(self.h, int(contig), int(side)), contig)

    def cmp_counts_diploid(self, contig: int, exact: bool = False) -> tuple:
        """The contig's truth diploid table scored against its calls one: (uint64[8, CMP_BINS, 6] -- truth matched, truth
        genotype-mismatched, truth missed, calls matched, calls genotype-mismatched, calls extra; uint64[2] as ``cmp_counts``)."""
        return self._cmp_counts(self.lib.msim_cmp_counts_diploid, 6, contig, exact)

    def cmp_fetch_diploid(self, contig: int, side: int, flags: bool = True) -> tuple:
        """(records, pool, genotype bytes, flag bytes) of one side's diploid table; the flags are those of the contig's last
        ``cmp_counts_diploid`` (0 no partner, 1 matched, 2 matched with another dosage; None with ``flags=False``)."""
        n, m = C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_cmp_fetch_diploid(self.h, int(contig), int(side), C.byref(n), C.byref(m), None, None, None, None),
                    contig)
        recs = np.zeros(n.value, dtype=RECORD_DTYPE)
        pool = np.zeros(m.value, dtype=np.uint8)
        gt = np.zeros(n.value, dtype=np.uint8)
        fl = np.zeros(n.value, dtype=np.uint8) if flags else None
        self._check(self.lib.msim_cmp_fetch_diploid(self.h, int(contig), int(side), None, None, _ptr(recs), _ptr(pool), _ptr(gt),
                                                    _ptr(fl) if flags else None), contig)
        return recs, pool, gt, fl

    def cmp_join_timing(self) -> float:
        """The diploid join's milliseconds on the device since ``reset_stats`` (HIP events)."""
        a = C.c_double()
        self._check(self.lib.msim_cmp_join_timing(self.h, C.byref(a)))
        return a.value

    def cmp_phase_mark(self, contig: int, side: int, haplotype: int) -> np.ndarray:
        """Directly behind a consensus-grammar ``vcf_plan_contig`` of the contig: the phase word of every record of the table just
        planned, kept as the marks of (contig, side, haplotype); uint64[3]: phased, unphased, unreadable-PS records."""
        tally = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.msim_cmp_phase_mark(self.h, int(contig), int(side), int(haplotype), _ptr(tally)), contig)
        return tally

    def cmp_phase_join(self, contig: int, side: int):
        """Behind ``cmp_join`` of that side: the diploid table's records get their phase words from the two haplotypes' marks,
        which are consumed."""
        self._check(self.lib.msim_cmp_phase_join(self.h, int(contig), int(side)), contig)

    def cmp_phase_set(self, contig: int, side: int, words):
        """The phase words of the side's diploid table, given directly (uint32, one per record)."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        self._check(self.lib.msim_cmp_phase_set(self.h, int(contig), int(side), _opt_ptr(words), len(words)), contig)

    def cmp_phase_counts(self, contig: int, exact: bool = False) -> np.ndarray:
        """Behind ``cmp_counts_diploid`` with the same ``exact``: uint64[CMP_PHASE_COUNTS] -- truth phased hets, calls phased
        hets, pairs, blocks, blocks of one pair, assessed adjacencies, raw switch bits, switches, flips, Hamming, pairs in blocks
        of two or more."""
        out = np.zeros(CMP_PHASE_COUNTS, dtype=np.uint64)
        self._check(self.lib.msim_cmp_phase_counts(self.h, int(contig), CMP_EXACT if exact else 0, _ptr(out)), contig)
        return out

    def cmp_fetch_phase(self, contig: int, side: int, state: bool = True) -> tuple:
        """(phase words, state bytes) of one side's diploid table, both sides joined; the state bytes are the truth's, of the contig's last
        ``cmp_phase_counts`` (0 not informative, 1 informative, +2 a raw switch bit, +4 orientation 1; None with ``state=False``)."""
        n = C.c_uint64()
        self._check(self.lib.msim_cmp_fetch_diploid(self.h, int(contig), int(side), C.byref(n), None, None, None, None, None), contig)
        words = np.zeros(n.value, dtype=np.uint32)
        st = np.zeros(n.value, dtype=np.uint8) if state else None
        self._check(self.lib.msim_cmp_fetch_phase(self.h, int(contig), int(side), _ptr(words), _ptr(st) if state else None), contig)
        return words, st

    def cmp_phase_timing(self) -> float:
        """The phase kernels' milliseconds on the device since ``reset_stats`` (HIP events)."""
        a = C.c_double()
        self._check(self.lib.msim_cmp_phase_timing(self.h, C.byref(a)))
        return a.value

    @staticmethod
    def _region_flags(exact: bool, diploid: bool) -> int:
        return (CMP_EXACT if exact else 0) | (CMP_DIPLOID if diploid else 0)

    def cmp_regions_set(self, contig: int, set_index: int, starts, ends):
        """Region set ``set_index`` (0 .. CMP_REGION_SETS - 1) of the contig: half-open 0-based intervals in normal form (sorted,
        merged, inside the contig); an empty list is the empty set.  The contig's marks are forgotten."""
        starts, ends = np.ascontiguousarray(starts, dtype=np.uint32), np.ascontiguousarray(ends, dtype=np.uint32)
        if len(starts) != len(ends):
            raise ValueError("cmp_regions_set: as many starts as ends")
        self._check(self.lib.msim_cmp_regions_set(self.h, int(contig), int(set_index), _opt_ptr(starts), _opt_ptr(ends), len(starts)), contig)

    def cmp_regions_drop(self, contig: int = -1, set_index: int = -1):
        """Drops one region set (``set_index`` -1: all of the contig's; ``contig`` -1: every contig's) and the marks."""
        self._check(self.lib.msim_cmp_regions_drop(self.h, int(contig), int(set_index)))

    def cmp_regions_mark(self, contig: int, exact: bool = False, diploid: bool = False):
        """A mark byte per record of the contig's held and current table (``diploid``: its two diploid tables): bit s set iff the
        record's anchor -- an indel's leftmost placement, else its pos -- lies inside resident set s."""
        self._check(self.lib.msim_cmp_regions_mark(self.h, int(contig), self._region_flags(exact, diploid)), contig)

    def cmp_counts_regions(self, contig: int, mask: int, exact: bool = False, diploid: bool = False, width: int | None = None) -> tuple:
        """Behind ``cmp_regions_mark`` and the count call whose flag bytes it tallies again, both with the same ``exact``: (that
        call's counts over the records inside every set of ``mask`` only, uint64[2]: the truth's and the calls' records outside).
        ``width``: the last axis of that call's counts, 4 (``cmp_counts``) or 6 (``cmp_counts_blocks``, ``cmp_counts_diploid``;
        the default with ``diploid``) -- the rows beyond a haploid count's 4 stay zero."""
        counts = np.zeros((8, CMP_BINS, 6), dtype=np.uint64)
        outside = np.zeros(2, dtype=np.uint64)
        self._check(self.lib.msim_cmp_counts_regions(self.h, int(contig), self._region_flags(exact, diploid), int(mask), _ptr(counts),
                                                     _ptr(outside)), contig)
        width = (6 if diploid else 4) if width is None else int(width)
        if width == 4:                                     # (written as [8][CMP_BINS][4] into the front of the buffer)
            counts = counts.reshape(-1)[:8 * CMP_BINS * 4].reshape(8, CMP_BINS, 4).copy()
        return counts, outside

    def cmp_fetch_regions(self, contig: int, exact: bool = False, diploid: bool = False) -> tuple:
        """(the truth's mark bytes, the calls') of the last ``cmp_regions_mark`` of these tables: one per record."""
        n = [C.c_uint64(), C.c_uint64()]
        if diploid:
            for side in (CMP_TRUTH, CMP_CALLS):
                self._check(self.lib.msim_cmp_fetch_diploid(self.h, int(contig), side, C.byref(n[side]), None, None, None, None, None), contig)
        else:
            self._check(self.lib.msim_cmp_fetch(self.h, int(contig), C.byref(n[0]), None, None, None, None, None), contig)
            n[1] = C.c_uint64(self.result_sizes(contig, applied=False)[1])
        a, b = np.zeros(n[0].value, dtype=np.uint8), np.zeros(n[1].value, dtype=np.uint8)
        self._check(self.lib.msim_cmp_fetch_regions(self.h, int(contig), self._region_flags(exact, diploid), _opt_ptr(a), _opt_ptr(b)), contig)
        return a, b

    def cmp_regions_timing(self) -> float:
        """The region kernels' milliseconds on the device since ``reset_stats`` (HIP events)."""
        a = C.c_double()
        self._check(self.lib.msim_cmp_regions_timing(self.h, C.byref(a)))
        return a.value

    # test hooks (msim_dbg_*: exported, not part of include/msim.h)
    def set_records(self, contig: int, recs: np.ndarray, pool: np.ndarray, with_offsets: bool = False):
        """Install a hand-built record table (RECORD_DTYPE) and insert pool on a contig, as the host planner installs its
        own.  The library checks the table first and raises MsimError (ERR_ARG) for one the kernels are not written for.
        ``with_offsets``: the output offsets come with the table (APPLY skips the device scan; needed for apply_batch)."""
        fn = self.lib.msim_dbg_set_records
        fn.restype, fn.argtypes = C.c_int, [_VP, C.c_int, _VP, C.c_uint64, _VP, C.c_uint64, C.c_uint32]
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        self._check(fn(self.h, contig, _ptr(recs), len(recs), _ptr(pool), len(pool), 1 if with_offsets else 0), contig)

    def apply_batch(self, contigs):
        """APPLY of several contigs whose tables came with their offsets as ONE batch (one tile-index launch, one rewrite
        launch per kernel variant), as the host-chain engines' deferred groups go out."""
        fn = self.lib.msim_dbg_apply_batch
        fn.restype, fn.argtypes = C.c_int, [_VP, _IP, C.c_int]
        ids = (C.c_int * len(contigs))(*[int(i) for i in contigs])
        self._check(fn(self.h, ids, len(contigs)))

    def emit_train(self, jobs, d: int = 1, train: int = 3):
        """The SNP sampler's emission train (count, expansion: one group's launches, ``train`` = 3 or 6) over the caller's
        bitmaps.  ``jobs``: up to 8 of (bitmap as uint64 words, start, contig length, aux8 = SNP outcomes by rank, at least
        one per set bit).  Returns (tile, [(records, first)]): each job's record table (RECORD_DTYPE) and, for train 3, its
        APPLY tile index (int32, ceil(length / tile) + 1 entries; None for train 6)."""
        fn = self.lib.msim_dbg_emit_train
        fn.restype = C.c_int
        fn.argtypes = [_VP, C.c_int, _VP, _VP, _VP, _VP, _VP, C.c_uint32, C.c_int, _VP, _VP, _VP, _VP]
        self.lib.msim_dbg_apply_tile.restype = C.c_uint32
        tile = int(self.lib.msim_dbg_apply_tile())
        n = len(jobs)
        bms = [np.ascontiguousarray(j[0], dtype=np.uint64) for j in jobs]
        auxs = [np.ascontiguousarray(j[3], dtype=np.uint8) for j in jobs]
        caps = [max(1, int(a.shape[0])) for a in auxs]
        auxs = [a if a.shape[0] else np.zeros(1, dtype=np.uint8) for a in auxs]
        recs = [np.zeros(cap, dtype=RECORD_DTYPE) for cap in caps]
        ptrs = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        n_words = np.array([b.shape[0] for b in bms], dtype=np.uint32)
        start = np.array([int(j[1]) for j in jobs], dtype=np.uint32)
        length = np.array([int(j[2]) for j in jobs], dtype=np.uint64)
        cap_a = np.array(caps, dtype=np.uint64)
        n_recs = np.zeros(n, dtype=np.uint64)
        n_tiles = [(int(j[2]) + tile - 1) // tile for j in jobs]
        firsts = [np.zeros(nt + 1, dtype=np.int32) for nt in n_tiles] if train == 3 else None
        self._check(fn(self.h, n, ptrs(bms), _ptr(n_words), _ptr(start), _ptr(length), ptrs(auxs), int(d), int(train),
                       ptrs(recs), _ptr(cap_a), _ptr(n_recs), ptrs(firsts) if firsts else None))
        return tile, [(recs[i][:int(n_recs[i])], firsts[i] if firsts and n_tiles[i] else None) for i in range(n)]

    def snp_draws(self, words, ti_lim: int, start: int, K: int, aux_off: int = 0):
        """The SNP ti/tv transducer over the caller's RAW CPython-stream ``words``: map pass over the whole blocks of 8192
        words, the scan for the end of ``K`` SNPs' draws from word ``start``, the outcome pass (msim_dbg_snp_draws).  Returns a
        dict: lanes (blocks + 1, 256, 4) uint32 = A, B, T, packed map per lane, maps (blocks + 1, 4) uint32 = counts from
        the three start states and end states per block -- the last block of both is a guard of 0xee bytes --, end_pos,
        flags, and aux = ``aux_off`` guard bytes, the K outcomes by rank, 16 guard bytes."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        n_blocks = words.shape[0] // 8192
        lanes = np.zeros((n_blocks + 1, 256, 4), dtype=np.uint32)
        maps = np.zeros((n_blocks + 1, 4), dtype=np.uint32)
        aux = np.zeros(int(aux_off) + int(K) + 16, dtype=np.uint8)
        end_pos, flags = C.c_uint64(0), C.c_uint32(0)
        self._check(self.lib.msim_dbg_snp_draws(self.h, _ptr(words), words.shape[0], int(ti_lim), int(start), int(K), int(aux_off),
                                                _ptr(lanes), _ptr(maps), C.byref(end_pos), C.byref(flags), _ptr(aux)))
        return {"lanes": lanes, "maps": maps, "end_pos": int(end_pos.value), "flags": int(flags.value), "aux": aux}

    def sample_tail(self, words, acc, acc_first: int, blocks, raw_counts: bool, W: int, shift: int, n: int, k: int, bitmap,
                    state: dict, win=None, pos_limit: int = 2 ** 64 - 1, guard: int = 4):
        """One launch of the sampler's tail rounds and stream cut over the caller's tables (msim_dbg_sample_tail): RAW
        CPython-stream ``words``, the accepted draws ``acc`` from accepted index ``acc_first`` on, ``blocks`` = the accepted
        draws per 2048-word block (``raw_counts``) or their exclusive prefix sums, the initial ``bitmap`` of ceil(n / 32) uint32
        and the initial ``state`` (pos, snp_base, flags, dups, accepted_used).  ``win`` = (pos, need0, d1): the anchored form.
        Returns (state, bitmap) -- the bitmap between ``guard`` words of 0xee bytes on either side, as they came back."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        acc = np.ascontiguousarray(acc, dtype=np.uint32)
        blocks = np.ascontiguousarray(blocks, dtype=np.uint32)
        bm = np.concatenate([np.full(guard, 0xEEEEEEEE, dtype=np.uint32), np.ascontiguousarray(bitmap, dtype=np.uint32),
                             np.full(guard, 0xEEEEEEEE, dtype=np.uint32)])
        assert bm.shape[0] == 2 * guard + (int(n) + 31) // 32, "bitmap: ceil(n / 32) words"
        n_blocks = blocks.shape[0] - (0 if raw_counts else 1)
        st = np.zeros(1, dtype=TAIL_STATE_DTYPE)
        for f in ("pos", "snp_base", "flags", "dups", "accepted_used"):
            st[f] = int(state.get(f, 0))
        wpos, need0, d1 = win if win is not None else (0, 0, 0)
        self._check(self.lib.msim_dbg_sample_tail(self.h, _ptr(words), words.shape[0], _ptr(acc), acc.shape[0], int(acc_first),
                                                  _ptr(blocks), int(n_blocks), 1 if raw_counts else 0, int(W), int(shift), int(n),
                                                  int(k), _ptr(bm), int(guard), _ptr(st), 0 if win is None else 1, int(wpos),
                                                  int(need0), int(d1), int(pos_limit)))
        return {f: int(st[f][0]) for f in ("pos", "snp_base", "flags", "dups", "accepted_used")}, bm

    def chain_step(self, words, ti_lim: int, lo: int, F: int, hcnt, hacc, tail, cnt, bitmap, state: dict, K: int, k_core: int,
                   shift: int, n: int, W: int, W2: int, K2: int, G: int, fused: bool, core_dups: int = 0, core_flags: int = 0,
                   head_flags: int = 0, expect: int = 0, soft_half: int = 0, pos_limit: int = 2 ** 64 - 1,
                   snp_limit: int = 2 ** 64 - 1, guard: int = 4):
        """One anchored contig's whole stream chain over the caller's tables (msim_dbg_chain_step): fringe, tail rounds, stream
        cut, SNP scan and cut -- ``fused``: as the one launch the sampler sends, else as the three stand-alone launches.  RAW
        CPython-stream ``words``; the head interval is words[lo, lo + F) with its accepted draws per 2048-word block (``hcnt``)
        and in order, a 2048-entry segment per block (``hacc``); the window is words[lo + F, lo + F + W) with its accepted draws
        per block (``cnt``) and, from accepted index ``k_core`` on, in order (``tail``); ``bitmap``: ceil(n / 32) uint32.
        Returns a dict: state (pos, snp_base, flags, dups, accepted_used, margin), hdr (need0, d1, ticket word, 0), bitmap
        between ``guard`` words of 0xee bytes, win_maps (W2 // 8192 + 4, 4) uint32 with the totals entry at W2 // 8192 + 2 and a
        guard entry behind it (what no launch wrote: 0xee bytes), base."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        hcnt = np.ascontiguousarray(hcnt, dtype=np.uint32)
        hacc = np.ascontiguousarray(hacc, dtype=np.uint32)
        tail = np.ascontiguousarray(tail, dtype=np.uint32)
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        assert hcnt.shape[0] == (int(F) + 2047) // 2048 and cnt.shape[0] == (int(W) + 2047) // 2048, "a count per 2048-word block"
        bm = np.concatenate([np.full(guard, 0xEEEEEEEE, dtype=np.uint32), np.ascontiguousarray(bitmap, dtype=np.uint32),
                             np.full(guard, 0xEEEEEEEE, dtype=np.uint32)])
        assert bm.shape[0] == 2 * guard + (int(n) + 31) // 32, "bitmap: ceil(n / 32) words"
        win = np.zeros((int(W2) // 8192 + 4, 4), dtype=np.uint32)
        io = np.zeros(1, dtype=CHAIN_STEP_DTYPE)
        for f, v in (("lo", lo), ("expect", expect), ("pos_limit", pos_limit), ("snp_limit", snp_limit), ("ti_lim", ti_lim), ("F", F),
                     ("K", K), ("k_core", k_core), ("shift", shift), ("n", n), ("W", W), ("W2", W2), ("K2", K2), ("soft_half", soft_half),
                     ("G", G), ("core_dups", core_dups), ("core_flags", core_flags), ("head_flags", head_flags), ("bm_guard", guard),
                     ("fused", 1 if fused else 0)):
            io[f] = int(v)
        for f in ("pos", "snp_base", "flags", "dups", "accepted_used"):
            io["state"][f] = int(state.get(f, 0))
        io["state"]["rsv"] = int(state.get("margin", 0))
        self._check(self.lib.msim_dbg_chain_step(self.h, _ptr(words), words.shape[0], _ptr(hcnt), _ptr(hacc), hacc.shape[0], _ptr(tail),
                                                 tail.shape[0], _ptr(cnt), _ptr(bm), _ptr(win), _ptr(io)))
        st = {f: int(io["state"][f][0]) for f in ("pos", "snp_base", "flags", "dups", "accepted_used")}
        st["margin"] = int(io["state"]["rsv"][0])
        return {"state": st, "hdr": [int(x) for x in io["hdr"][0]], "bitmap": bm, "win_maps": win, "base": int(io["base"][0])}

    def chains_fused(self) -> int:
        """Fused chain launches this context's SNP sampler has sent since it was created (msim_dbg_chains_fused)."""
        n = C.c_uint64(0)
        self._check(self.lib.msim_dbg_chains_fused(self.h, C.byref(n)))
        return int(n.value)

    def candidates(self, np_words, sets, bitmap=None, start: int = 0, d: int = 1, K: int = 0, ranges=None, all: bool = False):
        """The candidate front of the SV-mix (``bitmap`` given: one range, ``sets`` one TYPE_TABLE_DTYPE entry) or host-chain
        engine (``K`` candidates over ``ranges``, a MIX_RANGE_DTYPE table, and up to 8 ``sets``), then the compaction of the
        chain's candidates (``all``: every candidate).  ``np_words``: RAW NumPy-stream words, two per candidate.  Returns a dict:
        cand_pos (None without a bitmap), cand_type, nsn_pos (None without a bitmap), nsn_type, nsn_rank, n_nsn."""
        fn = self.lib.msim_dbg_candidates
        fn.restype = C.c_int
        fn.argtypes = [_VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _VP, C.c_uint32, _VP, C.c_uint32, _VP, C.c_uint64,
                       C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _U32P, _U32P]
        words = np.ascontiguousarray(np_words, dtype=np.uint32)
        sets = np.ascontiguousarray(np.atleast_1d(sets), dtype=TYPE_TABLE_DTYPE)
        if bitmap is not None:
            bm = np.ascontiguousarray(bitmap, dtype=np.uint64)
            cap = int(np.unpackbits(bm.view(np.uint8)).sum())
            rt, n_draw = None, 0
        else:
            bm, cap = None, int(K)
            rt = np.ascontiguousarray(ranges, dtype=MIX_RANGE_DTYPE)
            n_draw = len(rt)
        room = max(cap, 1)
        cand_pos, nsn_pos, nsn_rank = (np.zeros(room, dtype=np.uint32) for _ in range(3))
        cand_type, nsn_type = (np.zeros(room, dtype=np.uint8) for _ in range(2))
        k_out, n_nsn = C.c_uint32(), C.c_uint32()
        self._check(fn(self.h, _ptr(bm) if bm is not None else None, len(bm) if bm is not None else 0, int(start), int(d), int(K),
                       _ptr(rt) if rt is not None else None, n_draw, _ptr(sets), len(sets), _ptr(words), len(words), 1 if all else 0,
                       _ptr(cand_pos), _ptr(cand_type), _ptr(nsn_pos), _ptr(nsn_type), _ptr(nsn_rank), cap, C.byref(k_out),
                       C.byref(n_nsn)))
        k, m = k_out.value, n_nsn.value
        return {"cand_pos": cand_pos[:k] if bm is not None else None, "cand_type": cand_type[:k],
                "nsn_pos": nsn_pos[:m] if bm is not None else None, "nsn_type": nsn_type[:m], "nsn_rank": nsn_rank[:m], "n_nsn": m}

    def accept_tables(self, raw_words, n: int, p0: int, classes):
        """Both accept-table kernels over RAW CPython-stream words [p0, p0 + n) for ``classes`` = [(shift, width)]: returns
        (k_accept_tables' table, k_accept_tables_ps' table), each of shape (n + 1, 1 << lg_rows); rows the kernels never write
        (>= len(classes)) are zero."""
        fn = self.lib.msim_dbg_accept_tables
        fn.restype, fn.argtypes = C.c_int, [_VP, _VP, C.c_uint64, C.c_uint64, C.c_uint32, _VP, _VP, C.c_uint32, _VP, _VP]
        words = np.ascontiguousarray(raw_words, dtype=np.uint32)
        sh = np.array([c[0] for c in classes], dtype=np.uint32)
        width = np.array([c[1] for c in classes], dtype=np.uint32)
        rows = 1 << chain_lg_rows(len(classes))
        T = np.full((int(n) + 1, rows), 0xdddddddd, dtype=np.uint32)
        T_ps = np.full((int(n) + 1, rows), 0xdddddddd, dtype=np.uint32)
        self._check(fn(self.h, _ptr(words), len(words), int(p0), int(n), _ptr(sh), _ptr(width), len(classes), _ptr(T), _ptr(T_ps)))
        return T, T_ps

    def mixed_emit(self, length: int, cand_pos, cand_type, ch_rank, ch_stop, np_words, ch_extra=None, ch_aux=None, ranges=None,
                   visit_from=None, sn_chained: bool = False):
        """Keep flags through records of the SV-mix / host-chain engines (k_stop_scatter ... k_pool_fill) over hand-built
        candidates and chain verdicts; ``block`` comes from ``set_params``.  ``np_words``: RAW NumPy-stream words for the insert
        pool.  Returns a dict: recs (RECORD_DTYPE), rec_off, sn_index, pool, n_rec, n_sn, pool_len, len_delta."""
        fn = self.lib.msim_dbg_mixed_emit
        fn.restype = C.c_int
        fn.argtypes = [_VP, C.c_uint64, C.c_uint32, _VP, _VP, C.c_uint32, _VP, _VP, _VP, _VP, C.c_uint32, _VP, _VP, C.c_uint32, _VP,
                       C.c_uint64, _VP, _VP, _VP, _VP, C.c_uint64, _VP, C.POINTER(C.c_int64)]
        pos = np.ascontiguousarray(cand_pos, dtype=np.uint32)
        typ = np.ascontiguousarray(cand_type, dtype=np.uint8)
        rank = np.ascontiguousarray(ch_rank, dtype=np.uint32)
        stop = np.ascontiguousarray(ch_stop, dtype=np.uint32)
        words = np.ascontiguousarray(np_words, dtype=np.uint32)
        extra = None if ch_extra is None else np.ascontiguousarray(ch_extra, dtype=np.uint32)
        aux = None if ch_aux is None else np.ascontiguousarray(ch_aux, dtype=np.uint8)
        rt = None if ranges is None else np.ascontiguousarray(ranges, dtype=MIX_RANGE_DTYPE)
        visit = None if visit_from is None else np.ascontiguousarray(visit_from, dtype=np.uint32)
        k = len(pos)
        assert len(typ) == k and len(stop) == len(rank)
        opt = lambda a: _ptr(a) if a is not None else None
        recs = np.zeros(max(k, 1), dtype=RECORD_DTYPE)
        rec_off, sn_index = np.zeros(max(k, 1), dtype=np.uint32), np.zeros(max(k, 1), dtype=np.uint32)
        cap_pool = len(words)
        pool = np.zeros(max(cap_pool, 1), dtype=np.uint8)
        counts = np.zeros(4, dtype=np.uint32)
        delta = C.c_int64()
        self._check(fn(self.h, int(length), k, _ptr(pos), _ptr(typ), len(rank), _ptr(rank), _ptr(stop), opt(extra), opt(aux),
                       0 if rt is None else len(rt), opt(rt), opt(visit), 1 if sn_chained else 0, _ptr(words), len(words), _ptr(recs),
                       _ptr(rec_off), _ptr(sn_index), _ptr(pool), cap_pool, _ptr(counts), C.byref(delta)))
        n_rec, n_sn, pool_len = (int(x) for x in counts[:3])
        return {"recs": recs[:n_rec], "rec_off": rec_off[:n_rec], "sn_index": sn_index[:n_sn], "pool": pool[:pool_len],
                "n_rec": n_rec, "n_sn": n_sn, "pool_len": pool_len, "len_delta": int(delta.value)}

    def key_error(self, contig: int):
        """(base, position) of the KeyError the contig's APPLY recorded, or None."""
        base, pos = C.c_uint8(), C.c_uint64()
        rc = self.lib.msim_sync(self.h)                    # collects asynchronous APPLYs (their KeyError words)
        if rc not in (OK, ERR_KEY):
            self._check(rc, contig)
        if self.lib.msim_key_error(self.h, contig, C.byref(base), C.byref(pos)) != OK:
            return None
        return chr(base.value), pos.value

    def render_vcf_device(self, contig: int, seq_name: str, guess: int = 0) -> np.ndarray:
        """VCF record lines of the contig rendered on the device (uint8 array of text).  With a size ``guess`` the
        text comes back in ONE synchronising call when it fits (the library keeps the rendered text, so a second
        call with the right size only copies)."""
        need = C.c_uint64()
        name = seq_name.encode("utf-8", "replace")
        if guess > 0:
            out = np.empty(guess, dtype=np.uint8)
            rc = self.lib.msim_render_vcf_device(self.h, contig, name, _ptr(out), guess, C.byref(need))
            if rc == OK:
                return out[:need.value]
            if rc != ERR_ARG or need.value <= guess:
                self._check(rc, contig)
        else:
            self._check(self.lib.msim_render_vcf_device(self.h, contig, name, None, 0, C.byref(need)), contig)
        out = np.empty(need.value, dtype=np.uint8)
        if need.value:
            self._check(self.lib.msim_render_vcf_device(self.h, contig, name, _ptr(out), need.value, C.byref(need)), contig)
        return out

    def render_chain_device(self, contig: int, t_name: str, q_name: str, chain_id: int) -> np.ndarray:
        """The planned contig's liftover chain (msim.h: msim_render_chain_device) rendered on the device, as a uint8 array of
        text; empty for a contig without an aligned base."""
        need = C.c_uint64()
        t, q = t_name.encode("utf-8", "replace"), q_name.encode("utf-8", "replace")
        self._check(self.lib.msim_render_chain_device(self.h, contig, t, q, int(chain_id), None, 0, C.byref(need)), contig)
        out = np.empty(need.value, dtype=np.uint8)
        if need.value:
            self._check(self.lib.msim_render_chain_device(self.h, contig, t, q, int(chain_id), _ptr(out), need.value,
                                                          C.byref(need)), contig)
        return out

    def chain_kernel_ms(self) -> float:
        """Device time (HIP events) of the chain kernels of the last ``render_chain_device`` rendering; the first call switches
        the measurement on and returns 0 (msim_dbg_chain_ms: exported, not part of include/msim.h)."""
        fn = self.lib.msim_dbg_chain_ms
        fn.restype, fn.argtypes = C.c_int, [_VP, C.POINTER(C.c_double)]
        ms = C.c_double()
        self._check(fn(self.h, C.byref(ms)))
        return ms.value

    def render_vcf_device_size(self, contig: int, seq_name: str) -> int:
        """Render the contig's VCF record lines on the device and report their size (the text stays in HBM for
        ``render_vcf_device_into``)."""
        need = C.c_uint64()
        self._check(self.lib.msim_render_vcf_device(self.h, contig, seq_name.encode("utf-8", "replace"), None, 0,
                                                    C.byref(need)), contig)
        return need.value

    def render_vcf_device_into(self, contig: int, seq_name: str, out: np.ndarray) -> int:
        """... and copy them into the caller's buffer -- any writable uint8 array, e.g. a mapped span of the output file."""
        need = C.c_uint64()
        self._check(self.lib.msim_render_vcf_device(self.h, contig, seq_name.encode("utf-8", "replace"), _ptr(out),
                                                    out.shape[0], C.byref(need)), contig)
        return need.value

    def fetch_sequence_framed_size(self, contig: int, bpl: int) -> int:
        need = C.c_uint64()
        self._check(self.lib.msim_fetch_sequence_framed(self.h, contig, bpl, None, 0, C.byref(need)), contig)
        return need.value

    def fetch_sequence_framed_into(self, contig: int, bpl: int, out: np.ndarray) -> int:
        need = C.c_uint64()
        self._check(self.lib.msim_fetch_sequence_framed(self.h, contig, bpl, _ptr(out), out.shape[0], C.byref(need)), contig)
        return need.value

    def file_wait(self):
        """Everything queued by the ``..._to_file`` calls is in its file (raises the first failure of a queued write)."""
        self._check(self.lib.msim_file_wait(self.h))

    # ------------------------------------------------------------------ BGZF output (msim.h: msim_bgzf_*)
    def bgzf_open(self, channel: int, fd: int):
        """Output channel ``channel`` (0 FASTA, 1 VCF) writes BGZF into the regular file ``fd`` from now on; the ``offset``
        of the ``..._to_file`` calls on it is the uncompressed stream's length."""
        self._check(self.lib.msim_bgzf_open(self.h, int(channel), int(fd)))

    def bgzf_append(self, channel: int, data) -> None:
        """Host bytes appended to the channel's uncompressed stream (copied: ``data`` may be reused at once)."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if buf.shape[0]:
            self._check(self.lib.msim_bgzf_append(self.h, int(channel), C.c_void_p(buf.ctypes.data), buf.shape[0]))

    def bgzf_close(self, channel: int):
        """Tail + EOF marker out, channel joined; returns (compressed bytes, uncompressed bytes)."""
        c, u = C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_bgzf_close(self.h, int(channel), C.byref(c), C.byref(u)))
        return c.value, u.value

    def bgzf_compress(self, data, timed: bool = False):
        """``data`` (bytes-like) as a whole BGZF file, compressed on the device; ``timed``: (bytes, kernel ms)."""
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        n = int(buf.shape[0])
        cap = int(self.lib.msim_bgzf_bound(n))
        out = np.empty(cap, dtype=np.uint8)
        got, ms = C.c_uint64(), C.c_float()
        self._check(self.lib.msim_bgzf_compress(self.h, C.c_void_p(buf.ctypes.data) if n else None, n,
                                                C.c_void_p(out.ctypes.data), cap, C.byref(got), C.byref(ms) if timed else None))
        res = out[:got.value].tobytes()
        return (res, ms.value) if timed else res

    # ------------------------------------------------------------------ BGZF input (msim.h: msim_bgzf_probe / _inflate)
    def bgzf_inflate(self, data, out: np.ndarray | None = None, timed: bool = False):
        """A whole BGZF file (bytes-like) inflated on the device.  ``out`` (uint8, at least the probe's byte count; best a
        ``host_buffer``): filled, and the view ``out[:n]`` is returned; without it the result is a ``bytes`` object.
        ``timed``: (result, kernel ms).  ``MsimError`` with ``code == ERR_VALUE`` for bytes that are not BGZF and for a
        member that does not decode (the message names the member's file offset and the reason)."""
        buf = _as_u8(data)
        n = int(buf.shape[0])
        total, _ = bgzf_probe(buf)
        dst = np.empty(total, dtype=np.uint8) if out is None else out
        if dst.dtype != np.uint8 or dst.ndim != 1 or not dst.flags.c_contiguous or not dst.flags.writeable:
            raise ValueError("out must be a writable contiguous uint8 array")
        got, ms = C.c_uint64(), C.c_float()
        rc = self.lib.msim_bgzf_inflate(self.h, C.c_void_p(buf.ctypes.data) if n else None, n,
                                        C.c_void_p(dst.ctypes.data) if dst.shape[0] else None, int(dst.shape[0]),
                                        C.byref(got), C.byref(ms) if timed else None)
        if rc == ERR_VALUE:
            raise _bgzf_error(rc, self.lib.msim_last_error(self.h).decode())
        self._check(rc)
        res = dst[:got.value].tobytes() if out is None else dst[:got.value]
        return (res, ms.value) if timed else res

    def fetch_sequence_framed_to_file(self, contig: int, bpl: int, fd: int, offset: int) -> int:
        """The framed body QUEUED for bytes [offset, offset + n) of the open regular file ``fd`` (libmsim's output channel
        writes it while the caller goes on; ``file_wait`` / ``sync`` / ``close`` join); returns n.  ``MsimUnsupported``:
        ``fd`` is no regular file -- use ``..._into`` + write()."""
        n = C.c_uint64()
        self._check(self.lib.msim_fetch_sequence_framed_file(self.h, contig, bpl, int(fd), int(offset), C.byref(n)), contig)
        return n.value

    def render_vcf_device_to_file(self, contig: int, seq_name: str, fd: int, offset: int) -> int:
        """The contig's VCF record lines into bytes [offset, offset + n) of the open file ``fd``; returns n."""
        n = C.c_uint64()
        self._check(self.lib.msim_render_vcf_device_file(self.h, contig, seq_name.encode("utf-8", "replace"), int(fd),
                                                         int(offset), C.byref(n)), contig)
        return n.value

    def fetch_sequence_framed(self, contig: int, bpl: int, guess_len: int | None = None) -> np.ndarray:
        """The mutated contig as FASTA body text (newline after every ``bpl`` bases).  With ``guess_len`` (e.g. the
        input length: an SNP-only table never changes it) the text comes back in ONE synchronising call when it
        fits; the library keeps the framed text, so a retry with the exact size only copies."""
        need = C.c_uint64()
        if guess_len is not None:
            cap = guess_len + guess_len // bpl + guess_len // 8 + 64
            out = np.empty(cap, dtype=np.uint8)
            rc = self.lib.msim_fetch_sequence_framed(self.h, contig, bpl, _ptr(out), cap, C.byref(need))
            if rc == OK:
                return out[:need.value]
            if rc != ERR_ARG or need.value <= cap:
                self._check(rc, contig)
        else:
            self._check(self.lib.msim_fetch_sequence_framed(self.h, contig, bpl, None, 0, C.byref(need)), contig)
        out = np.empty(need.value, dtype=np.uint8)
        if need.value:
            self._check(self.lib.msim_fetch_sequence_framed(self.h, contig, bpl, _ptr(out), need.value, C.byref(need)), contig)
        return out

    def result_checksum(self, contig: int) -> int:
        s = C.c_uint64()
        self._check(self.lib.msim_result_checksum(self.h, contig, C.byref(s)))
        return s.value

    def result_device_ptr(self, contig: int):
        """(device address, length) of the mutated stream, for GPU-to-GPU transports."""
        a, n = C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_result_device_ptr(self.h, contig, C.byref(a), C.byref(n)), contig)
        return a.value, n.value

    # ------------------------------------------------------------------ many small contigs in one pass
    def batch_run(self, items):
        """``items``: list of (body uint8 array, n_bases, lenc, lenb, [Range], name, header).  Returns (fasta_text, vcf_text,
        per-contig empty flags, bases on the last FASTA line): the texts are uint8 VIEWS of libmsim's buffers (valid until
        the next batch); fasta_text is the complete run of records ('>' header lines included) as FastaWriter writes them."""
        n = len(items)
        arr = (BatchContig * n)()
        keep = []
        for i, (body, n_bases, lenc, lenb, ranges, name, header) in enumerate(items):
            body = np.ascontiguousarray(body, dtype=np.uint8)
            ra = (Range * max(len(ranges), 1))(*ranges)
            nm = name.encode("utf-8", "replace")
            hd = header.encode("utf-8", "replace")
            keep.append((body, ra, nm, hd))
            q = arr[i]
            q.body = body.ctypes.data
            q.body_bytes = body.shape[0]
            q.n_bases = n_bases
            q.lenc, q.lenb = lenc, lenb
            q.ranges = ra
            q.n_ranges = len(ranges)
            q.name = nm
            q.header = hd
        self._check(self.lib.msim_batch_run(self.h, arr, n))
        return self._batch_result(n)          # (frames the FASTA text now: the deflines in `keep` die with this call)

    def batch_run_table(self, table: np.ndarray, keep=(), defer_fasta: bool = False):
        """The same from a ready ``BATCH_CONTIG_DTYPE`` table (pointers into buffers the caller keeps alive -- ``keep`` --
        for the duration of the call): an assembly's batch is built with array operations, not per contig.
        ``defer_fasta``: the first result is the FASTA text's SIZE; ``batch_fetch_fasta(dst)`` then frames it straight into
        ``dst`` (a mapped span of the output file) -- the deflines the table points at must still be alive then."""
        table = np.ascontiguousarray(table)
        n = int(table.shape[0])
        self._check(self.lib.msim_batch_run(self.h, C.cast(C.c_void_p(table.ctypes.data), C.POINTER(BatchContig)), n))
        del keep
        return self._batch_result(n, defer_fasta)

    def batch_fetch_fasta(self, dst: np.ndarray):
        """Frame the last batch's FASTA text into ``dst`` (writable, contiguous uint8, at least the text's size)."""
        if dst.dtype != np.uint8 or not dst.flags.c_contiguous or not dst.flags.writeable:
            raise ValueError("batch_fetch_fasta needs a writable contiguous uint8 array")
        self._check(self.lib.msim_batch_fetch(self.h, C.c_void_p(dst.ctypes.data), dst.shape[0], None, 0))

    def batch_fetch_to_files(self, fasta_fd: int, fasta_offset: int, vcf_fd: int, vcf_offset: int):
        """Queue the last batch's FASTA text (framed by libmsim's host threads) and VCF text for their files' spans at the
        given offsets (-1: not that one); ``file_wait`` joins."""
        self._check(self.lib.msim_batch_fetch_file(self.h, int(fasta_fd), int(fasta_offset), int(vcf_fd), int(vcf_offset)))

    def _batch_result(self, n: int, defer_fasta: bool = False):
        em = (C.c_int32 * n)()
        self._check(self.lib.msim_batch_sizes(self.h, n, None, None, em, None))
        fp, vp = C.c_void_p(), C.c_void_p()
        fn, vn, last = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.msim_batch_view(self.h, None if defer_fasta else C.byref(fp), C.byref(fn), C.byref(vp), C.byref(vn),
                                             C.byref(last)))

        def view(ptr, nbytes):
            if not nbytes:
                return np.empty(0, dtype=np.uint8)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))
        return (fn.value if defer_fasta else view(fp, fn.value)), view(vp, vn.value), np.frombuffer(em, dtype=np.int32) != 0, last.value

    # ------------------------------------------------------------------ multi-GPU (csrc/comm.cpp)
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self.lib.msim_comm_init(self.h, buf, rank, world))

    def comm_destroy(self):
        self._check(self.lib.msim_comm_destroy(self.h))

    def planned_out_len(self, contig: int):
        """(mutated length, known): known = PLAN alone fixes the length (every rank can compute it)."""
        n, k = C.c_uint64(), C.c_int()
        self._check(self.lib.msim_planned_out_len(self.h, contig, C.byref(n), C.byref(k)))
        return n.value, bool(k.value)

    def gather_to_root(self, contig_ids, owner, out_len, n_records=None, pool_len=None, root: int = 0):
        """Moves every slot -- mutated stream, and with ``n_records`` / ``pool_len`` its record table and insert pool -- to
        ``root`` over RCCL; returns per slot the device addresses (stream, records, pool) on this rank (0: not here / empty)."""
        n = len(contig_ids)
        ids = (C.c_int * max(n, 1))(*contig_ids)
        own = (C.c_int * max(n, 1))(*owner)
        lens = (C.c_uint64 * max(n, 1))(*out_len)
        nrec = (C.c_uint64 * max(n, 1))(*n_records) if n_records is not None else None
        pool = (C.c_uint64 * max(n, 1))(*pool_len) if pool_len is not None else None
        addrs = (C.c_uint64 * (3 * max(n, 1)))()
        self._check(self.lib.msim_gather_to_root(self.h, n, ids, own, lens, nrec, pool, root, addrs))
        return [tuple(addrs[3 * i + j] for j in range(3)) for i in range(n)]

    def gather_fetch(self, device_addr: int, nbytes: int, dtype=np.uint8) -> np.ndarray:
        """A gathered part (address from ``gather_to_root``) as a host array."""
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if nbytes:
            self._check(self.lib.msim_gather_fetch(self.h, device_addr, nbytes, C.c_void_p(out.ctypes.data)))
        return out

    def release_result(self, contig: int):
        self._check(self.lib.msim_release_result(self.h, contig))

    def stats(self) -> dict:
        t = Timing()
        self._check(self.lib.msim_stats(self.h, C.byref(t)))
        return t.as_dict()

    def reset_stats(self):
        self._check(self.lib.msim_reset_stats(self.h))


def comm_unique_id() -> bytes:
    """ncclGetUniqueId as 128 opaque bytes (call on one rank, broadcast over the control plane)."""
    lib = load()
    # RCCL's bootstrap looks for a network interface; on a box without one (or without name resolution) that can
    # take a minute.  Inside one node the loopback interface is all it needs.
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_IB_DISABLE", "1")
    buf = (C.c_uint8 * 128)()
    rc = lib.msim_comm_unique_id(buf)
    if rc != OK:
        raise MsimError(f"msim_comm_unique_id failed ({rc}): {lib.msim_last_error(None).decode()}")
    return bytes(buf)


def gather_plan(owner, out_len, rank: int, world: int, root: int = 0, n_records=None, pool_len=None):
    """The transfers ``rank`` posts for a gather: list of (kind, slot, part, peer, bytes); kind 0 send, 1 recv, 2 local;
    part 0 the mutated stream, 1 the record table, 2 the insert pool."""
    lib = load()
    n = len(owner)
    own = (C.c_int * max(n, 1))(*owner)
    lens = (C.c_uint64 * max(n, 1))(*out_len)
    nrec = (C.c_uint64 * max(n, 1))(*n_records) if n_records is not None else None
    pool = (C.c_uint64 * max(n, 1))(*pool_len) if pool_len is not None else None
    ops = (C.c_int64 * (15 * max(n, 1)))()
    k = C.c_int()
    rc = lib.msim_gather_plan(n, own, lens, nrec, pool, rank, world, root, ops, C.byref(k))
    if rc != OK:
        raise MsimError(f"msim_gather_plan failed ({rc})")
    return [tuple(int(ops[5 * i + j]) for j in range(5)) for i in range(k.value)]


def render_vcf(recs: np.ndarray, pool: np.ndarray, bases: np.ndarray, seq_name: str) -> bytes:
    """Record table -> VCF record lines (host helper; no GPU, no context)."""
    lib = load()
    recs = np.ascontiguousarray(recs)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    need = C.c_uint64()
    name = seq_name.encode("utf-8", "replace")
    rc = lib.msim_render_vcf(_ptr(recs), recs.shape[0], _ptr(pool), _ptr(bases), bases.shape[0],
                             name, None, 0, C.byref(need))
    if rc != OK:
        raise MsimError(f"msim_render_vcf failed ({rc})")
    out = np.empty(need.value, dtype=np.uint8)
    rc = lib.msim_render_vcf(_ptr(recs), recs.shape[0], _ptr(pool), _ptr(bases), bases.shape[0],
                             name, _ptr(out), need.value, C.byref(need))
    if rc != OK:
        raise MsimError(f"msim_render_vcf failed ({rc})")
    return out.tobytes()


def render_vcf_gt(recs: np.ndarray, gt, pool: np.ndarray, bases: np.ndarray, seq_name: str) -> bytes:
    """``msim_render_vcf_gt``: the record lines with the phased genotype column of ``gt`` (one byte per record, 1..3; None: the
    haploid column of ``render_vcf``).  Host helper; no GPU, no context."""
    lib = load()
    recs = np.ascontiguousarray(recs)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    g = None if gt is None else np.ascontiguousarray(gt, dtype=np.uint8)
    if g is not None and g.shape[0] != recs.shape[0]:
        raise MsimError("render_vcf_gt: one genotype byte per record")
    need = C.c_uint64()
    name = seq_name.encode("utf-8", "replace")
    gp = None if g is None else _ptr(g)
    rc = lib.msim_render_vcf_gt(_ptr(recs), gp, recs.shape[0], _ptr(pool), _ptr(bases), bases.shape[0], name, None, 0, C.byref(need))
    if rc != OK:
        err = MsimError(f"msim_render_vcf_gt failed ({rc})")
        err.code = rc
        raise err
    out = np.empty(need.value, dtype=np.uint8)
    rc = lib.msim_render_vcf_gt(_ptr(recs), gp, recs.shape[0], _ptr(pool), _ptr(bases), bases.shape[0], name, _ptr(out), need.value,
                                C.byref(need))
    if rc != OK:
        raise MsimError(f"msim_render_vcf_gt failed ({rc})")
    return out.tobytes()


def hap_block() -> int:
    """Records of a workgroup of the haplotype compaction kernels (csrc/haplotype.hip: HAP_BLOCK), where their edge cases lie
    (msim_dbg_hap_block: exported, not part of include/msim.h)."""
    fn = load().msim_dbg_hap_block
    fn.restype, fn.argtypes = C.c_uint32, []
    return int(fn())


def _thr_array(thr) -> np.ndarray:
    thr = np.array([int(x) for x in thr], dtype=np.uint64) if not isinstance(thr, np.ndarray) else np.ascontiguousarray(thr, dtype=np.uint64)
    if thr.shape != (192,):
        raise ValueError("a spectrum has 192 thresholds (64 contexts x 3 alternative bases)")
    return thr


def _host_error(rc: int) -> MsimError:
    err = (MsimUnsupported if rc == ERR_UNSUPPORTED else MsimError)(f"libmsim error {rc}: {load().msim_last_error(None).decode()}")
    err.code = rc
    return err


def context_counts_host(bases) -> tuple:
    """``msim_dbg_context_counts``: the census of ``Engine.context_counts`` by a sequential host loop over ``bases`` (uint8,
    upper-cased).  No context, no GPU."""
    lib = load()
    bases = _as_u8(bases)
    counts = np.zeros(64, dtype=np.uint64)
    n = C.c_uint64()
    rc = lib.msim_dbg_context_counts(C.c_void_p(bases.ctypes.data) if len(bases) else None, len(bases), _ptr(counts), C.byref(n))
    if rc != OK:
        raise _host_error(rc)
    return counts, n.value


def spectrum_plan_host(bases, thr, key: int, seq: int) -> np.ndarray:
    """``msim_dbg_spectrum_plan``: the record table ``Engine.plan_contig_spectrum`` leaves (RECORD_DTYPE), by a sequential host
    loop.  No context, no GPU."""
    lib = load()
    bases = _as_u8(bases)
    thr = _thr_array(thr)
    src = C.c_void_p(bases.ctypes.data) if len(bases) else None
    n = C.c_uint64()
    key = int(key) & (2**64 - 1)
    rc = lib.msim_dbg_spectrum_plan(src, len(bases), _ptr(thr), key, int(seq), None, 0, C.byref(n))
    if rc != OK:
        raise _host_error(rc)
    recs = np.zeros(n.value, dtype=RECORD_DTYPE)
    if n.value:
        rc = lib.msim_dbg_spectrum_plan(src, len(bases), _ptr(thr), key, int(seq), _ptr(recs), n.value, C.byref(n))
        if rc != OK:
            raise _host_error(rc)
    return recs


def sbs_counts_host(bases, recs) -> tuple:
    """``msim_dbg_sbs_counts``: what ``Engine.sbs_counts`` returns, by a sequential host loop over ``bases`` (uint8, upper-cased)
    and ``recs`` (RECORD_DTYPE).  No context, no GPU."""
    lib = load()
    bases = _as_u8(bases)
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
    channels = np.zeros(SBS_CHANNELS, dtype=np.uint64)
    tallies = np.zeros(SBS_TALLIES, dtype=np.uint64)
    rc = lib.msim_dbg_sbs_counts(C.c_void_p(bases.ctypes.data) if len(bases) else None, len(bases),
                                 C.c_void_p(recs.ctypes.data) if len(recs) else None, len(recs), _ptr(channels), _ptr(tallies))
    if rc != OK:
        raise _host_error(rc)
    return channels, tallies


def _opt_ptr(a):
    return C.c_void_p(a.ctypes.data) if len(a) else None


def _cmp_counts_host(bases, truth, calls, exact: bool) -> tuple:
    """The two sequential restatements' call: ``truth`` and ``calls`` are (records, pool) -- ``msim_dbg_cmp_counts`` -- or
    (records, pool, genotype bytes) -- ``msim_dbg_cmp_counts_diploid``."""
    lib = load()
    bases = _as_u8(bases)
    diploid = len(truth) == 3
    sides = []
    for recs, *rest in (truth, calls):
        side = [np.ascontiguousarray(recs, dtype=RECORD_DTYPE)] + [np.ascontiguousarray(a, dtype=np.uint8) for a in rest]
        assert all(len(gt) == len(side[0]) for gt in side[2:])
        sides.append(side)
    counts = np.zeros((8, CMP_BINS, 6 if diploid else 4), dtype=np.uint64)
    tallies = np.zeros(2, dtype=np.uint64)
    fa = np.zeros(len(sides[0][0]), dtype=np.uint8)
    fb = np.zeros(len(sides[1][0]), dtype=np.uint8)
    args = [_opt_ptr(bases), len(bases)]
    for recs, pool, *gt in sides:
        args += [_opt_ptr(recs), len(recs), _opt_ptr(pool), len(pool)] + [_opt_ptr(a) for a in gt]
    rc = (lib.msim_dbg_cmp_counts_diploid if diploid else lib.msim_dbg_cmp_counts)(
        *args, CMP_EXACT if exact else 0, _ptr(counts), _ptr(tallies), _opt_ptr(fa), _opt_ptr(fb))
    if rc != OK:
        raise _host_error(rc)
    return counts, tallies, fa, fb


def cmp_counts_host(bases, truth, truth_pool, calls, calls_pool, exact: bool = False) -> tuple:
    """``msim_dbg_cmp_counts``: what ``Engine.cmp_counts`` returns and the two flag arrays of ``Engine.cmp_fetch`` -- (counts,
    tallies, truth flags, calls flags) -- by a sequential host loop over ``bases`` (uint8, upper-cased) and two tables
    (RECORD_DTYPE, insert pools uint8).  No context, no GPU."""
    return _cmp_counts_host(bases, (truth, truth_pool), (calls, calls_pool), exact)


def cmp_counts_blocks_host(bases, truth, truth_pool, calls, calls_pool, exact: bool = False, gap: int = CMP_BLOCK_GAP) -> tuple:
    """``msim_dbg_cmp_counts_blocks``: what ``Engine.cmp_counts_blocks`` returns and the two flag arrays of ``Engine.cmp_fetch``
    behind it -- (counts, tallies, block tallies, truth flags, calls flags) -- by sequential host loops.  No context, no GPU."""
    lib = load()
    bases = _as_u8(bases)
    truth, calls = (np.ascontiguousarray(t, dtype=RECORD_DTYPE) for t in (truth, calls))
    truth_pool, calls_pool = (np.ascontiguousarray(p, dtype=np.uint8) for p in (truth_pool, calls_pool))
    counts = np.zeros((8, CMP_BINS, 6), dtype=np.uint64)
    tallies = np.zeros(2, dtype=np.uint64)
    blocks = np.zeros(5, dtype=np.uint64)
    fa = np.zeros(len(truth), dtype=np.uint8)
    fb = np.zeros(len(calls), dtype=np.uint8)
    rc = lib.msim_dbg_cmp_counts_blocks(_opt_ptr(bases), len(bases), _opt_ptr(truth), len(truth), _opt_ptr(truth_pool), len(truth_pool),
                                        _opt_ptr(calls), len(calls), _opt_ptr(calls_pool), len(calls_pool), CMP_EXACT if exact else 0,
                                        int(gap), _ptr(counts), _ptr(tallies), _ptr(blocks), _opt_ptr(fa), _opt_ptr(fb))
    if rc != OK:
        raise _host_error(rc)
    return counts, tallies, blocks, fa, fb


def cmp_join_host(h1, pool1, h2, pool2) -> tuple:
    """``msim_dbg_cmp_join``: the diploid table ``Engine.cmp_join`` makes of two haplotype tables -- (records, pool, genotype
    bytes) -- by a sequential host merge.  No context, no GPU."""
    lib = load()
    h1 = np.ascontiguousarray(h1, dtype=RECORD_DTYPE)
    h2 = np.ascontiguousarray(h2, dtype=RECORD_DTYPE)
    pool1 = np.ascontiguousarray(pool1, dtype=np.uint8)
    pool2 = np.ascontiguousarray(pool2, dtype=np.uint8)
    out = np.zeros(len(h1) + len(h2), dtype=RECORD_DTYPE)
    gt = np.zeros(len(h1) + len(h2), dtype=np.uint8)
    pool = np.zeros(len(pool1) + len(pool2), dtype=np.uint8)
    n = C.c_uint64()
    rc = lib.msim_dbg_cmp_join(_opt_ptr(h1), len(h1), _opt_ptr(pool1), len(pool1), _opt_ptr(h2), len(h2), _opt_ptr(pool2), len(pool2),
                               _opt_ptr(out), _opt_ptr(pool), _opt_ptr(gt), C.byref(n))
    if rc != OK:
        raise _host_error(rc)
    return out[:n.value].copy(), pool, gt[:n.value].copy()


def cmp_counts_diploid_host(bases, truth, truth_pool, truth_gt, calls, calls_pool, calls_gt, exact: bool = False) -> tuple:
    """``msim_dbg_cmp_counts_diploid``: what ``Engine.cmp_counts_diploid`` returns and the two flag arrays of
    ``Engine.cmp_fetch_diploid`` -- (counts, tallies, truth flags, calls flags) -- by a sequential host loop over two diploid
    tables with a genotype byte per record.  No context, no GPU."""
    return _cmp_counts_host(bases, (truth, truth_pool, truth_gt), (calls, calls_pool, calls_gt), exact)


VCF_GROUP_DTYPE = np.dtype([("name_off", "<u8"), ("first_line", "<u8"), ("n_lines", "<u8"), ("name_len", "<u4"), ("rsv", "<u4")])   # msim_vcf_group
FASTA_RECORD_DTYPE = np.dtype([("h0", "<u8"), ("h1", "<u8"), ("b0", "<u8"), ("b1", "<u8"), ("n_bases", "<u8"),
                               ("lenc", "<u4"), ("lenb", "<u4"), ("flags", "<u4"), ("rsv", "<u4")])   # msim_fasta_record
FASTA_HAS_BODY, FASTA_BAD_LINES, FASTA_NONUNIFORM = 1, 2, 4


def cmp_phase_host(bases, truth, truth_pool, truth_gt, truth_words, calls, calls_pool, calls_gt, calls_words, exact: bool = False) -> tuple:
    """``msim_dbg_cmp_phase``: what ``Engine.cmp_phase_counts`` returns and the truth's state bytes of ``Engine.cmp_fetch_phase``
    by sequential host loops over two diploid tables with their genotype bytes and phase words.  No context, no GPU."""
    lib = load()
    bases = _as_u8(bases)
    args = [_opt_ptr(bases), len(bases)]
    n = []
    for recs, pool, gt, words in ((truth, truth_pool, truth_gt, truth_words), (calls, calls_pool, calls_gt, calls_words)):
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        pool, gt = np.ascontiguousarray(pool, dtype=np.uint8), np.ascontiguousarray(gt, dtype=np.uint8)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert len(gt) == len(recs) == len(words)
        args += [_opt_ptr(recs), len(recs), _opt_ptr(pool), len(pool), _opt_ptr(gt), _opt_ptr(words)]
        n.append((recs, pool, gt, words))                  # (kept alive over the call)
    out = np.zeros(CMP_PHASE_COUNTS, dtype=np.uint64)
    state = np.zeros(len(n[0][0]), dtype=np.uint8)
    rc = lib.msim_dbg_cmp_phase(*args, CMP_EXACT if exact else 0, _ptr(out), _opt_ptr(state))
    if rc != OK:
        raise _host_error(rc)
    return out, state


def cmp_counts_regions_host(bases, truth, truth_pool, truth_flags, calls, calls_pool, calls_flags, outcomes: int, sets, mask: int,
                            exact: bool = False) -> tuple:
    """``msim_dbg_cmp_counts_regions``: what ``Engine.cmp_counts_regions`` and ``Engine.cmp_fetch_regions`` return -- (counts,
    outside, truth marks, calls marks) -- by sequential host loops.  The flag bytes are those of the count call with ``outcomes``
    (2 or 3) outcomes; ``sets``: up to CMP_REGION_SETS pairs (starts, ends).  No context, no GPU."""
    lib = load()
    bases = _as_u8(bases)
    truth, calls = (np.ascontiguousarray(t, dtype=RECORD_DTYPE) for t in (truth, calls))
    truth_pool, calls_pool, truth_flags, calls_flags = (np.ascontiguousarray(p, dtype=np.uint8)
                                                        for p in (truth_pool, calls_pool, truth_flags, calls_flags))
    assert len(truth_flags) == len(truth) and len(calls_flags) == len(calls)
    sets = [(np.ascontiguousarray(s, dtype=np.uint32), np.ascontiguousarray(e, dtype=np.uint32)) for s, e in sets]
    assert all(len(s) == len(e) for s, e in sets)
    starts = np.concatenate([s for s, _ in sets] + [np.zeros(0, dtype=np.uint32)])
    ends = np.concatenate([e for _, e in sets] + [np.zeros(0, dtype=np.uint32)])
    off = np.zeros(len(sets) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s, _ in sets], dtype=np.uint64)
    counts = np.zeros((8, CMP_BINS, 2 * int(outcomes) if outcomes in (2, 3) else 6), dtype=np.uint64)
    outside = np.zeros(2, dtype=np.uint64)
    ma, mb = np.zeros(len(truth), dtype=np.uint8), np.zeros(len(calls), dtype=np.uint8)
    rc = lib.msim_dbg_cmp_counts_regions(_opt_ptr(bases), len(bases), _opt_ptr(truth), len(truth), _opt_ptr(truth_pool), len(truth_pool),
                                         _opt_ptr(truth_flags), _opt_ptr(calls), len(calls), _opt_ptr(calls_pool), len(calls_pool),
                                         _opt_ptr(calls_flags), int(outcomes), CMP_EXACT if exact else 0, len(sets), _opt_ptr(starts),
                                         _opt_ptr(ends), _ptr(off), int(mask), _ptr(counts), _ptr(outside), _opt_ptr(ma), _opt_ptr(mb))
    if rc != OK:
        raise _host_error(rc)
    return counts, outside, ma, mb


def bed_scan(text) -> tuple:
    """``msim_bed_scan``: BED text (bytes or uint8) in one sequential pass -- (starts uint32, ends uint32, 1-based lines uint64 per
    kept interval; per run of consecutive kept lines with one name: name offset uint64, name length uint32, first interval uint64,
    count uint64).  MsimError with code ERR_VALUE and ``BED line N: reason`` for the first offending line."""
    lib = load()
    text = _as_u8(text)
    n_iv, n_run = C.c_uint64(0), C.c_uint64(0)
    rc = lib.msim_bed_scan(_opt_ptr(text), len(text), None, None, None, C.byref(n_iv), None, None, None, None, C.byref(n_run))
    if rc != OK:
        raise _host_error(rc)
    starts, ends = np.zeros(n_iv.value, dtype=np.uint32), np.zeros(n_iv.value, dtype=np.uint32)
    lines = np.zeros(n_iv.value, dtype=np.uint64)
    name_off, name_len = np.zeros(n_run.value, dtype=np.uint64), np.zeros(n_run.value, dtype=np.uint32)
    first, count = np.zeros(n_run.value, dtype=np.uint64), np.zeros(n_run.value, dtype=np.uint64)
    if n_iv.value:
        rc = lib.msim_bed_scan(_ptr(text), len(text), _ptr(starts), _ptr(ends), _ptr(lines), C.byref(n_iv), _ptr(name_off), _ptr(name_len),
                               _ptr(first), _ptr(count), C.byref(n_run))
        if rc != OK:
            raise _host_error(rc)
    return starts, ends, lines, name_off, name_len, first, count


def vcf_phase_word(line: bytes, nf0: int, sample: int = 0) -> tuple:
    """``msim_dbg_vcf_phase_word``: (the phase word of one VCF line of a file with ``nf0`` fields a line, sample column ``sample``;
    whether its PS was unreadable)."""
    lib = load()
    buf = np.frombuffer(bytes(line), dtype=np.uint8)
    word, bad = C.c_uint32(), C.c_uint32()
    rc = lib.msim_dbg_vcf_phase_word(_opt_ptr(buf), len(buf), int(nf0), int(sample), C.byref(word), C.byref(bad))
    if rc != OK:
        raise _host_error(rc)
    return word.value, bool(bad.value)


def _as_u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return np.frombuffer(data, dtype=np.uint8)


def _bgzf_error(rc: int, msg: str) -> MsimError:
    e = MsimError(f"libmsim error {rc}: {msg}")
    e.code = rc
    return e


def bgzf_probe(data):
    """(uncompressed bytes, members) of a BGZF file given as bytes-like, from a host pass over its member chain (no
    device, no context); empty members count.  ``MsimError`` with ``code == ERR_VALUE``: not gzip, gzip without BGZF
    framing, a BSIZE past the end, a truncated member."""
    lib = load()
    buf = _as_u8(data)
    n = int(buf.shape[0])
    total, members = C.c_uint64(), C.c_uint64()
    rc = lib.msim_bgzf_probe(C.c_void_p(buf.ctypes.data) if n else None, n, C.byref(total), C.byref(members))
    if rc != OK:
        raise _bgzf_error(rc, lib.msim_last_error(None).decode())
    return total.value, members.value


def fasta_index(text: np.ndarray):
    """Index pass over a whole FASTA text (uint8): structured array of msim_fasta_record, or None when sequence text
    precedes the first defline (pyfaidx: FastaIndexingError)."""
    lib = load()
    text = np.ascontiguousarray(text, dtype=np.uint8)
    n = C.c_uint64()
    cap = 4096                                         # one pass for anything but a large assembly (the defline scan reads
    while True:                                        # the whole text: do not run it twice just to learn the count)
        out = np.zeros(cap, dtype=FASTA_RECORD_DTYPE)
        rc = lib.msim_fasta_index(_ptr(text), text.shape[0], out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        if rc == 3:                                    # MSIM_ERR_VALUE
            return None
        if rc == ERR_ARG and n.value > cap:
            cap = n.value
            continue
        if rc:
            raise MsimError(f"msim_fasta_index failed ({rc})")
        out = out[:n.value]
        break
    return out
