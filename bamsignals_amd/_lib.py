"""ctypes binding of libbamsignals_hip.so (the C ABI declared in include/bamsignals_abi.h).

The product path has no CPU fallback: if the shared object is missing this module raises at
import of the first symbol, and every compute call needs a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BSIG_LIB_PATH selects another build of the same ABI (the diagnostic stamps build); never a fallback
SO_PATH = os.environ.get("BSIG_LIB_PATH") or os.path.join(_HERE, "libbamsignals_hip.so")

BSIG_OK = 0
MODE_PROFILE, MODE_COUNT, MODE_COVERAGE, MODE_COVERAGE_EX = 0, 1, 2, 3
# bamOverlaps: Params.binsize carries minoverlap in these modes
MODE_OVERLAP_ANY, MODE_OVERLAP_WITHIN = 4, 5
# include/bamsignals_abi.h: BSIG_XCORR_MAX_LAG, BSIG_XCORR_MOMENTS
XCORR_MAX_LAG, XCORR_MOMENTS = 2047, 5
# include/bamsignals_abi.h: BSIG_FRAG_MAX_ROWS
FRAG_MAX_ROWS = 16384
# include/bamsignals_abi.h: BSIG_VPLOT_MAX_CELLS
VPLOT_MAX_CELLS = 1 << 24
# include/bamsignals_abi.h: BSIG_HIST_MAX_ROWS, BSIG_HIST_MOMENTS
HIST_MAX_ROWS, HIST_MOMENTS = 8192, 2
# include/bamsignals_abi.h: BSIG_SUMMARY_FIXED, BSIG_SUMMARY_MAX_THRESHOLDS
SUMMARY_FIXED, SUMMARY_MAX_THRESHOLDS = 3, 8
# include/bamsignals_abi.h: BSIG_SCALED_MAX_BINS
SCALED_MAX_BINS = 2048
# the largest keep_dup (keepDup): an int32
KEEP_DUP_MAX = 2**31 - 1

ERR_NAMES = {-1: "BSIG_ERR_ARG", -2: "BSIG_ERR_IO", -3: "BSIG_ERR_NOINDEX", -4: "BSIG_ERR_CHROM",
             -5: "BSIG_ERR_EXT", -6: "BSIG_ERR_DEVICE", -7: "BSIG_ERR_NOMEM", -8: "BSIG_ERR_FORMAT"}


class BsigError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code
        self.code_name = ERR_NAMES.get(code, str(code))


class Columns(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_ref", C.c_int32), ("ref_len", C.c_void_p),
                ("ref_off", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p),
                ("mapq", C.c_void_p), ("tlen", C.c_void_p), ("end", C.c_void_p),
                ("cigar_off", C.c_void_p), ("cigar", C.c_void_p)]


class BaseColumns(C.Structure):
    # bsig_base_columns: seq_off counts bases; base g is nibble g of seq (the high half of byte g / 2 where g is even), byte g of qual
    _fields_ = [("seq_off", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p)]


class ReadsInfo(C.Structure):
    # classes 0..3 by span, 4 = the packed class (include/bamsignals_abi.h: BSIG_N_CLASSES)
    _fields_ = [("n_reads", C.c_int64), ("hbm_bytes", C.c_int64), ("n_classes", C.c_int32), ("n_codes", C.c_int32),
                ("class_n", C.c_int64 * 5), ("class_maxspan", C.c_int32 * 5),
                ("class_bucket_shift", C.c_int32 * 5)]


class Params(C.Structure):
    _fields_ = [("mode", C.c_int32), ("mapqual", C.c_int32), ("binsize", C.c_int32),
                ("shift", C.c_int32), ("ss", C.c_int32), ("requiredF", C.c_int32),
                ("filteredF", C.c_int32), ("pe_mid", C.c_int32), ("tspan", C.c_int32),
                ("n_tlen_filter", C.c_int32), ("tlen_filter", C.c_int32 * 2),
                ("tile_cells", C.c_int32), ("threads", C.c_int32)]


class PlanStats(C.Structure):
    _fields_ = [("n_ranges", C.c_int64), ("n_items", C.c_int64), ("cells", C.c_int64),
                ("visits", C.c_int64), ("visits_short", C.c_int64), ("streamed", C.c_int64),
                ("algorithmic_bytes", C.c_int64), ("bytes_per_visit_short", C.c_int32),
                ("bytes_per_visit_long", C.c_int32), ("visits_packed", C.c_int64),
                ("bytes_per_visit_packed", C.c_int32), ("heavy_tiles", C.c_int32)]


_lib = None


def load():
    """Load the HIP shared object.  torch (when importable) is imported first so that both use
    the one libamdhip64 the process already holds."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C bamsignals_amd/csrc`.  bamsignals_amd has no CPU fallback.")
    try:  # noqa: SIM105
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, not a requirement
        pass
    lib = C.CDLL(SO_PATH)
    lib.bsig_last_error.restype = C.c_char_p
    lib.bsig_layout.restype = C.c_int64
    lib.bsig_layout.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.bsig_ctx_create.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.bsig_ctx_destroy.argtypes = [C.c_void_p]
    lib.bsig_ctx_destroy.restype = None
    lib.bsig_ctx_sync.argtypes = [C.c_void_p]
    lib.bsig_ctx_stream.argtypes = [C.c_void_p]
    lib.bsig_ctx_stream.restype = C.c_void_p
    lib.bsig_host_alloc.argtypes = [C.c_int64, C.POINTER(C.c_void_p)]
    lib.bsig_host_free.argtypes = [C.c_void_p]
    lib.bsig_host_free.restype = None
    lib.bsig_reads_upload.argtypes = [C.c_void_p, C.POINTER(Columns), C.POINTER(C.c_void_p)]
    lib.bsig_reads_get_info.argtypes = [C.c_void_p, C.POINTER(ReadsInfo)]
    # spliced reads (rows = aligned blocks): made from CIGAR columns or from a BAM, told apart by bsig_reads_is_spliced
    # (BSIG_LIB_PATH may name a build from before them, as for bsig_overlap_core below)
    if hasattr(lib, "bsig_reads_upload_spliced"):
        lib.bsig_reads_upload_spliced.argtypes = lib.bsig_reads_upload.argtypes
        lib.bsig_reads_is_spliced.argtypes = [C.c_void_p]
        lib.bsig_reads_is_spliced.restype = C.c_int32
    lib.bsig_reads_clone.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.bsig_reads_free.argtypes = [C.c_void_p]
    lib.bsig_reads_free.restype = None
    lib.bsig_reads_save.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.bsig_reads_load.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.bsig_last_call_route.restype = C.c_char_p
    lib.bsig_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(C.c_void_p)]
    # plans of reads resized to the fragment: the fragment length between the parameters and the handle
    # (BSIG_LIB_PATH may name a build from before them, as for bsig_overlap_core below)
    for name in ("bsig_plan_create_resized", "bsig_plan_create_sum_resized"):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = lib.bsig_plan_create.argtypes[:-1] + [C.c_int32, C.POINTER(C.c_void_p)]
    lib.bsig_plan_offsets.argtypes = [C.c_void_p]
    lib.bsig_plan_offsets.restype = C.POINTER(C.c_int64)
    lib.bsig_plan_cells.argtypes = [C.c_void_p]
    lib.bsig_plan_cells.restype = C.c_int64
    lib.bsig_plan_get_stats.argtypes = [C.c_void_p, C.POINTER(PlanStats)]
    lib.bsig_plan_run.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_plan_run_host.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_plan_run_host_async.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_plan_overflowed.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.bsig_plan_free.argtypes = [C.c_void_p]
    lib.bsig_plan_free.restype = None
    # the reduction plans: (kind, has an int32 argument of its own, has a runs query)
    for kind, extra, runs in (("sum", False, False), ("xcorr", True, False), ("frag", True, True), ("hist", True, True)):
        create = lib.bsig_plan_create.argtypes
        getattr(lib, f"bsig_plan_create_{kind}").argtypes = create[:-1] + [C.c_int32, create[-1]] if extra else create
        for query in ("cells", "runs") if runs else ("cells",):
            getattr(lib, f"bsig_plan_{kind}_{query}").argtypes = [C.c_void_p]
            getattr(lib, f"bsig_plan_{kind}_{query}").restype = C.c_int64
        getattr(lib, f"bsig_plan_run_{kind}").argtypes = [C.c_void_p, C.c_void_p]
        getattr(lib, f"bsig_plan_run_{kind}_host").argtypes = [C.c_void_p, C.c_void_p]
    # ... and the vplot plan: its own argument is the row width; rows, columns and the kernel's form beside cells and runs
    lib.bsig_plan_create_vplot.argtypes = lib.bsig_plan_create.argtypes[:-1] + [C.c_int32, C.POINTER(C.c_void_p)]
    for query, restype in (("cells", C.c_int64), ("runs", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("form", C.c_int32)):
        getattr(lib, f"bsig_plan_vplot_{query}").argtypes = [C.c_void_p]
        getattr(lib, f"bsig_plan_vplot_{query}").restype = restype
    lib.bsig_plan_run_vplot.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_plan_run_vplot_host.argtypes = [C.c_void_p, C.c_void_p]
    # ... and the summary plan: its own arguments are the number of thresholds and the thresholds
    lib.bsig_plan_create_summary.argtypes = lib.bsig_plan_create.argtypes[:-1] + [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    for query in ("cells", "runs"):
        getattr(lib, f"bsig_plan_summary_{query}").argtypes = [C.c_void_p]
        getattr(lib, f"bsig_plan_summary_{query}").restype = C.c_int64
    lib.bsig_plan_run_summary.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_plan_run_summary_host.argtypes = [C.c_void_p, C.c_void_p]
    # ... and the scaled plan: its own argument is the number of bins
    lib.bsig_plan_create_scaled.argtypes = lib.bsig_plan_create.argtypes[:-1] + [C.c_int32, C.POINTER(C.c_void_p)]
    for query in ("cells", "runs"):
        getattr(lib, f"bsig_plan_scaled_{query}").argtypes = [C.c_void_p]
        getattr(lib, f"bsig_plan_scaled_{query}").restype = C.c_int64
    lib.bsig_plan_scaled_segmented.argtypes = [C.c_void_p]
    lib.bsig_plan_scaled_segmented.restype = C.c_int32
    lib.bsig_plan_run_scaled.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_plan_run_scaled_host.argtypes = [C.c_void_p, C.c_void_p]
    # ... and the capped plan: keep_dup and frag_len
    lib.bsig_plan_create_capped.argtypes = lib.bsig_plan_create.argtypes[:-1] + [C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    for query in ("cells", "runs"):
        getattr(lib, f"bsig_plan_capped_{query}").argtypes = [C.c_void_p]
        getattr(lib, f"bsig_plan_capped_{query}").restype = C.c_int64
    lib.bsig_plan_run_capped.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_plan_run_capped_host.argtypes = [C.c_void_p, C.c_void_p]
    lib.bsig_runs_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.bsig_runs_n_seg.argtypes = [C.c_void_p]
    lib.bsig_runs_n_seg.restype = C.c_int64
    lib.bsig_runs_cells.argtypes = [C.c_void_p]
    lib.bsig_runs_cells.restype = C.c_int64
    lib.bsig_runs_encode.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.bsig_runs_device.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p)]
    lib.bsig_runs_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsig_runs_free.argtypes = [C.c_void_p]
    lib.bsig_runs_free.restype = None
    lib.bsig_plan_runs_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.bsig_views_create.argtypes = lib.bsig_runs_create.argtypes
    lib.bsig_views_n_seg.argtypes = [C.c_void_p]
    lib.bsig_views_n_seg.restype = C.c_int64
    lib.bsig_views_cells.argtypes = [C.c_void_p]
    lib.bsig_views_cells.restype = C.c_int64
    lib.bsig_views_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    lib.bsig_views_device.argtypes = [C.c_void_p, C.POINTER(C.c_int64)] + [C.POINTER(C.c_void_p)] * 6
    lib.bsig_views_fetch.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    lib.bsig_views_free.argtypes = [C.c_void_p]
    lib.bsig_views_free.restype = None
    lib.bsig_plan_views_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.bsig_pileup_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p]
    lib.bsig_bam_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.bsig_bam_close.argtypes = [C.c_void_p]
    lib.bsig_bam_close.restype = None
    lib.bsig_bam_path.argtypes = [C.c_void_p]
    lib.bsig_bam_path.restype = C.c_char_p
    lib.bsig_reads_from_bam.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.bsig_reads_from_bam_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_int32)]
    lib.bsig_reads_from_bam_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int32, C.POINTER(C.c_void_p)]
    if hasattr(lib, "bsig_reads_from_bam_spliced"):
        lib.bsig_reads_from_bam_spliced.argtypes = lib.bsig_reads_from_bam.argtypes
        lib.bsig_reads_from_bam_regions_spliced.argtypes = lib.bsig_reads_from_bam_regions.argtypes
    lib.bsig_device_decode_timing.argtypes = [C.POINTER(C.c_double)]
    lib.bsig_device_decode_timing.restype = None
    lib.bsig_bam_n_ref.argtypes = [C.c_void_p]
    lib.bsig_bam_ref_name.argtypes = [C.c_void_p, C.c_int32]
    lib.bsig_bam_ref_name.restype = C.c_char_p
    lib.bsig_bam_ref_len.argtypes = [C.c_void_p, C.c_int32]
    lib.bsig_bam_name2id.argtypes = [C.c_void_p, C.c_char_p]
    lib.bsig_bam_decode.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.POINTER(Columns)]
    core_head = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_void_p, C.c_int32]
    lib.bsig_bam_decode_timing.argtypes = [C.POINTER(C.c_double)]
    lib.bsig_bam_decode_timing.restype = None
    lib.bsig_pileup_core.argtypes = core_head + [C.c_int32] * 9 + [C.c_void_p, C.c_void_p]
    lib.bsig_coverage_core.argtypes = core_head + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]
    # (BSIG_LIB_PATH may name a build from before bamOverlaps -- the yardstick of scripts/overlaps_times.py --, which
    # lacks this one entry: bamOverlaps then raises AttributeError where it would call it)
    if hasattr(lib, "bsig_overlap_core"):
        lib.bsig_overlap_core.argtypes = core_head + [C.c_int32] * 9 + [C.c_void_p, C.c_void_p]
    lib.bsig_pileup_core_into.argtypes = core_head + [C.c_int32] * 9 + [C.c_void_p]
    lib.bsig_coverage_core_into.argtypes = core_head + [C.c_int32] * 6 + [C.c_void_p]
    lib.bsig_coverage_core_ex.argtypes = core_head + [C.c_int32] * 8 + [C.c_void_p, C.c_void_p]
    lib.bsig_coverage_core_ex_into.argtypes = core_head + [C.c_int32] * 8 + [C.c_void_p]
    lib.bsig_pileup_sum.argtypes = core_head + [C.c_int32] * 9 + [C.c_void_p]
    lib.bsig_coverage_sum.argtypes = core_head + [C.c_int32] * 8 + [C.c_void_p]
    lib.bsig_pileup_xcorr.argtypes = core_head + [C.c_int32] * 6 + [C.c_void_p]
    lib.bsig_pileup_frag.argtypes = core_head + [C.c_int32] * 7 + [C.c_void_p]
    lib.bsig_pileup_vplot.argtypes = core_head + [C.c_int32] * 8 + [C.c_void_p]
    lib.bsig_pileup_hist.argtypes = core_head + [C.c_int32] * 8 + [C.c_void_p]
    lib.bsig_coverage_hist.argtypes = core_head + [C.c_int32] * 7 + [C.c_void_p]
    lib.bsig_pileup_summary.argtypes = core_head + [C.c_int32] * 6 + [C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p]
    lib.bsig_coverage_summary.argtypes = core_head + [C.c_int32] * 5 + [C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p]
    lib.bsig_pileup_scaled.argtypes = core_head + [C.c_int32] * 8 + [C.c_void_p]
    lib.bsig_coverage_scaled.argtypes = core_head + [C.c_int32] * 7 + [C.c_void_p]
    # the capped signals: bsig_pileup_core's arguments with keep_dup behind pe_mid, bsig_coverage_core_ex's with frag_len and
    # keep_dup behind tspan
    lib.bsig_pileup_capped.argtypes = core_head + [C.c_int32] * 10 + [C.c_void_p, C.c_void_p]
    lib.bsig_coverage_capped.argtypes = core_head + [C.c_int32] * 10 + [C.c_void_p, C.c_void_p]
    lib.bsig_pileup_runs.argtypes = core_head + [C.c_int32] * 9 + [C.POINTER(C.c_void_p)]
    lib.bsig_coverage_runs.argtypes = core_head + [C.c_int32] * 8 + [C.POINTER(C.c_void_p)]
    # ... of reads resized to the fragment: frag_len in tspan's place
    if hasattr(lib, "bsig_coverage_core_resized"):
        lib.bsig_coverage_core_resized.argtypes = lib.bsig_coverage_core_ex.argtypes
        lib.bsig_coverage_sum_resized.argtypes = lib.bsig_coverage_sum.argtypes
        lib.bsig_coverage_runs_resized.argtypes = lib.bsig_coverage_runs.argtypes
    lib.bsig_runs_result_n_seg.argtypes = [C.c_void_p]
    lib.bsig_runs_result_n_seg.restype = C.c_int64
    lib.bsig_runs_result_n_runs.argtypes = [C.c_void_p]
    lib.bsig_runs_result_n_runs.restype = C.c_int64
    lib.bsig_runs_result_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsig_runs_result_free.argtypes = [C.c_void_p]
    lib.bsig_runs_result_free.restype = None
    # the views calls: the runs calls' arguments, then lower and upper
    lib.bsig_pileup_views.argtypes = core_head + [C.c_int32] * 11 + [C.POINTER(C.c_void_p)]
    lib.bsig_coverage_views.argtypes = core_head + [C.c_int32] * 10 + [C.POINTER(C.c_void_p)]
    lib.bsig_coverage_views_resized.argtypes = lib.bsig_coverage_views.argtypes
    # ... and of spliced reads: the same calls without tspan
    if hasattr(lib, "bsig_coverage_core_spliced"):
        lib.bsig_coverage_core_spliced.argtypes = core_head + [C.c_int32] * 7 + [C.c_void_p, C.c_void_p]
        lib.bsig_coverage_sum_spliced.argtypes = core_head + [C.c_int32] * 7 + [C.c_void_p]
        lib.bsig_coverage_runs_spliced.argtypes = core_head + [C.c_int32] * 7 + [C.POINTER(C.c_void_p)]
        lib.bsig_coverage_views_spliced.argtypes = core_head + [C.c_int32] * 9 + [C.POINTER(C.c_void_p)]
    # the junctions of spliced reads: the table's size, the query at handle level and at file level, the result handle
    # (BSIG_LIB_PATH may name a build from before them -- the yardstick of scripts/junctions_times.py)
    if hasattr(lib, "bsig_reads_junctions"):
        lib.bsig_reads_n_junction_rows.argtypes = [C.c_void_p]
        lib.bsig_reads_n_junction_rows.restype = C.c_int64
        lib.bsig_reads_junctions.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.POINTER(C.c_void_p)]
        lib.bsig_junctions.argtypes = core_head[:8] + [C.c_int32] * 6 + [C.POINTER(C.c_void_p)]
        lib.bsig_junctions_result_n_seg.argtypes = [C.c_void_p]
        lib.bsig_junctions_result_n_seg.restype = C.c_int64
        lib.bsig_junctions_result_n_junctions.argtypes = [C.c_void_p]
        lib.bsig_junctions_result_n_junctions.restype = C.c_int64
        lib.bsig_junctions_result_copy.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        lib.bsig_junctions_result_free.argtypes = [C.c_void_p]
        lib.bsig_junctions_result_free.restype = None
    # reads per gene: the host-side gene model, the read table's size, the query at handle level and at file level
    # (BSIG_LIB_PATH may name a build from before them -- the yardstick of scripts/genecounts_times.py)
    if hasattr(lib, "bsig_reads_gene_counts"):
        lib.bsig_gene_model_create.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_int32] * 2 + [C.POINTER(C.c_void_p)]
        lib.bsig_gene_model_free.argtypes = [C.c_void_p]
        lib.bsig_gene_model_free.restype = None
        lib.bsig_gene_model_n_genes.argtypes = [C.c_void_p]
        lib.bsig_gene_model_n_ref.argtypes = [C.c_void_p]
        lib.bsig_gene_model_n_segments.argtypes = [C.c_void_p, C.c_int32]
        lib.bsig_gene_model_n_segments.restype = C.c_int64
        lib.bsig_gene_model_copy_segments.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
        lib.bsig_reads_n_source_reads.argtypes = [C.c_void_p]
        lib.bsig_reads_n_source_reads.restype = C.c_int64
        lib.bsig_reads_gene_counts.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 2
        lib.bsig_gene_counts.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p)] + [C.c_int32] * 5 + [C.c_void_p] * 2
    # reads with bases and the nucleotide counts (BSIG_LIB_PATH may name a build from before them)
    if hasattr(lib, "bsig_reads_nucleotides"):
        lib.bsig_reads_upload_bases.argtypes = [C.c_void_p, C.POINTER(Columns), C.POINTER(BaseColumns), C.POINTER(C.c_void_p)]
        lib.bsig_reads_has_bases.argtypes = [C.c_void_p]
        lib.bsig_reads_has_bases.restype = C.c_int32
        lib.bsig_reads_base_table_bytes.argtypes = [C.c_void_p]
        lib.bsig_reads_base_table_bytes.restype = C.c_int64
        lib.bsig_bam_decode_bases.argtypes = lib.bsig_bam_decode.argtypes + [C.POINTER(BaseColumns)]
        lib.bsig_reads_from_bam_bases.argtypes = lib.bsig_reads_from_bam.argtypes
        lib.bsig_reads_from_bam_regions_bases.argtypes = lib.bsig_reads_from_bam_regions.argtypes
        lib.bsig_nucleotides_cells.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
        lib.bsig_nucleotides_cells.restype = C.c_int64
        lib.bsig_reads_nucleotides.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p]
        lib.bsig_reads_nucleotides_host.argtypes = lib.bsig_reads_nucleotides.argtypes
        lib.bsig_nucleotides.argtypes = core_head[:8] + [C.c_int32] * 6 + [C.c_void_p]
    # the sites among the nucleotide cells: the query at handle level and at file level, the result handle (BSIG_LIB_PATH may
    # name a build from before them -- the yardstick of scripts/sites_times.py)
    if hasattr(lib, "bsig_reads_sites"):
        lib.bsig_reads_sites.argtypes = ([C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.c_void_p] + [C.c_int32] * 5
                                         + [C.POINTER(C.c_void_p)])
        lib.bsig_sites.argtypes = core_head[:8] + [C.c_int32] * 5 + [C.c_void_p] + [C.c_int32] * 6 + [C.POINTER(C.c_void_p)]
        lib.bsig_sites_result_n_ranges.argtypes = [C.c_void_p]
        lib.bsig_sites_result_n_ranges.restype = C.c_int64
        lib.bsig_sites_result_n_sites.argtypes = [C.c_void_p]
        lib.bsig_sites_result_n_sites.restype = C.c_int64
        lib.bsig_sites_result_copy.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        lib.bsig_sites_result_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.bsig_sites_result_timing.restype = None
        lib.bsig_sites_result_free.argtypes = [C.c_void_p]
        lib.bsig_sites_result_free.restype = None
    lib.bsig_views_result_n_seg.argtypes = [C.c_void_p]
    lib.bsig_views_result_n_seg.restype = C.c_int64
    lib.bsig_views_result_n_views.argtypes = [C.c_void_p]
    lib.bsig_views_result_n_views.restype = C.c_int64
    lib.bsig_views_result_copy.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    lib.bsig_views_result_free.argtypes = [C.c_void_p]
    lib.bsig_views_result_free.restype = None
    lib.bsig_write_sam_as_bam_and_index.argtypes = [C.c_char_p, C.c_char_p]
    lib.bsig_write_columns_as_bam.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(Columns),
                                              C.c_int32]
    lib.bsig_write_columns_as_bam_with_seq.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(Columns),
                                                       C.c_int32, C.c_int32, C.c_uint64]
    lib.bsig_cache_clear.restype = None
    lib.bsig_debug_scratch_allocs.restype = C.c_int64
    lib.bsig_effective_cpus.restype = C.c_int32
    lib.bsig_debug_block_table.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    lib.bsig_debug_block_table_progressive.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    lib.bsig_segmap_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.bsig_segmap_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsig_segmap_free.argtypes = [C.c_void_p]
    lib.bsig_segmap_free.restype = None
    lib.bsig_narrow_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.bsig_narrow_bytes.restype = C.c_int64
    lib.bsig_narrow_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    lib.bsig_narrow_count.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.bsig_segmap_run_narrow.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.bsig_segmap_narrow_overflowed.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.bsig_last_call_timing.argtypes = [C.POINTER(C.c_double)]
    lib.bsig_last_call_timing.restype = None
    lib.bsig_last_call_timing_ex.argtypes = [C.POINTER(C.c_double), C.c_int32]
    lib.bsig_last_call_timing_ex.restype = None
    lib.bsig_check_list.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.bsig_check_list.restype = C.c_int32
    lib.bsig_fast_width.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    lib.bsig_fast_width.restype = None
    lib.bsig_scatter_segments.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def check(rc):
    if rc != BSIG_OK:
        raise BsigError(rc, load().bsig_last_error().decode("utf-8", "replace"))
