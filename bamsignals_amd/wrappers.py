"""bamCount / bamProfile / bamCoverage: the reference's user API (R/wrappers.R:75-184), with the
same argument names, defaults, normalisation, warnings, errors and return shapes, over the C ABI.

R is not available in the build image, so this Python module is the host side that can be run
and tested here.  Under R nothing of this is needed: the reference's own ``R/`` files stay as they
are and only ``src/`` is swapped (bamsignals_amd/r_package/graft_into_reference.sh).
``paired.end`` is spelled ``paired_end``.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import warnings

import numpy as np

from . import _lib
from .countsignals import CountSignals
from .granges import GRanges
from .runsignals import RunSignals


def _match_arg(value, choices, name):
    """R's match.arg: a vector of choices means the first one; unique prefixes are accepted."""
    if isinstance(value, (list, tuple)):
        if list(value) == list(choices):
            return choices[0]
        if len(value) != 1:
            raise ValueError(f"'{name}' must be of length 1")
        value = value[0]
    hits = [c for c in choices if c.startswith(str(value))] if value != "" else []
    if value in choices:
        return value
    if len(hits) != 1:
        raise ValueError(f"'{name}' should be one of " + ", ".join(f"‘{c}’" for c in choices))
    return hits[0]


def flagMask(paired_end):
    """R/wrappers.R:76-81: only the first read of a properly mapped pair (0x2 | 0x40) unless ignored."""
    return 66 if paired_end != "ignore" else 0


def tlenFilter(tlenFilter, paired_end):  # noqa: N802,N803 - reference names
    """R/wrappers.R:84-98."""
    if paired_end == "ignore":
        return ()
    if tlenFilter is None:
        return (0, 1000)
    tf = list(np.atleast_1d(tlenFilter))
    if len(tf) != 2 or tf[0] < 0 or tf[1] < 0:
        raise ValueError("tlenFilter must be NULL or vector of 2 positive integers")
    if tf[0] > tf[1]:
        raise ValueError("tlenFilter[1] must be smaller or equal to tlenFilter[2]")
    return (int(tf[0]), int(tf[1]))


def _print_sentence(path):
    """The reference prints a progress line per call when ``verbose`` (R/wrappers.R:175-184); only its
    presence matters, so the text here is a plain one."""
    print(f"Processing {path}", file=sys.stderr)


# GPU the file-level calls run on when the caller passes no ``device``: -1 = the library's own choice
# (env BAMSIGNALS_DEVICES, else BAMSIGNALS_DEVICE, else GPU 0).  One-process-per-GPU hosts
# (bamsignals_amd.dist) set it to their rank's GPU.
_default_device = -1


def set_default_device(device):
    """Make ``device`` (a GPU ordinal, or -1 for the library's choice) the default of bamCount /
    bamProfile / bamCoverage in this process."""
    global _default_device
    _default_device = int(device)


def _dev(device):
    return _default_device if device is None else int(device)


def _check_gr(gr):
    if not isinstance(gr, GRanges):
        raise TypeError("must provide a GRanges object")        # ref: src/bamsignals.cpp:93-94


class _Head(tuple):
    """The ten leading arguments of a file-level call -- path, n, the ranges' codes, the number of levels, their names,
    start, width, strand, the length filter and its count.  The arrays they point into live as long as it does;
    ``width`` and ``tf`` are the flattened widths and the filter as the call sees them."""


def _head(bampath, gr, tlen_filter):
    _check_gr(gr)
    levels, codes, start, width, strand = gr.flatten()
    tf = np.asarray([int(x) for x in tlen_filter], dtype=np.int32)
    names = (C.c_char_p * max(len(levels), 1))(*[s.encode() for s in levels])
    head = _Head((os.path.expanduser(str(bampath)).encode(), len(gr), codes.ctypes.data, len(levels), names,
                  start.ctypes.data, width.ctypes.data, strand.ctypes.data, tf.ctypes.data, len(tf)))
    head.keep, head.width, head.tf = (codes, start, strand), width, tf
    return head


def _split(out, off, ss):
    out.setflags(write=False)          # the signals are views of this buffer: read-only container
    n = len(off) - 1
    if n > 64:
        # ranges of one width (tilings, fixed windows around features): the rows of ONE reshaped view -- a million
        # per-range views cost 0.16 s this way, 0.35 s sliced one by one
        w = int(off[1] - off[0])
        if w > 0 and int(off[-1]) == n * w and bool(np.all(np.diff(off) == w)):
            if ss:
                return list(out[:n * w].reshape(n, w // 2, 2).transpose(0, 2, 1))
            return list(out[:n * w].reshape(n, w))
    off = off.tolist()
    if ss:
        return [out[a:b].reshape(-1, 2).T for a, b in zip(off[:-1], off[1:])]
    return [out[a:b] for a, b in zip(off[:-1], off[1:])]


def pileup_core(bampath, gr, tlen_filter, mapqual=0, binsize=1, shift=0, ss=False, requiredF=0,
                filteredF=-1, pe_mid=False, maxgap=16385, device=None):
    """The native entry point behind bamCount/bamProfile (ref: R/RcppExports.R:12-14).  Returns the
    R list as a Python list: per-range vectors / 2 x w matrices, or, for binsize <= 0, a list of
    length one holding the count vector / 2 x n matrix."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    n = len(gr)
    off = np.empty(n + 1, dtype=np.int64)
    cells = lib.bsig_layout(n, head.width.ctypes.data, int(binsize), int(bool(ss)), off.ctypes.data)
    out = np.zeros(cells, dtype=np.int32)
    _lib.check(lib.bsig_pileup_core(*head, int(mapqual), int(binsize), int(shift), int(bool(ss)), int(requiredF),
                                    int(filteredF), int(bool(pe_mid)), int(maxgap), _dev(device), out.ctypes.data,
                                    off.ctypes.data))
    if binsize <= 0:
        return [out.reshape(-1, 2).T if ss else out]
    return _split(out, off, ss)


def overlap_core(bampath, gr, tlen_filter, mapqual=0, within=False, min_overlap=1, ss=False, requiredF=0,
                 filteredF=-1, tspan=False, maxgap=16385, device=None):
    """The native entry point behind bamOverlaps (bsig_overlap_core): the int32 count vector, or the 2 x n matrix
    (sense, antisense) with ``ss``.  ``maxgap`` is there for the shape of the other entry points; the call ignores it."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    n = len(gr)
    off = np.empty(n + 1, dtype=np.int64)
    cells = lib.bsig_layout(n, head.width.ctypes.data, -1, int(bool(ss)), off.ctypes.data)
    out = np.zeros(cells, dtype=np.int32)
    _lib.check(lib.bsig_overlap_core(*head, int(mapqual), int(bool(within)), int(min_overlap), int(bool(ss)), int(requiredF),
                                     int(filteredF), int(bool(tspan)), int(maxgap), _dev(device), out.ctypes.data,
                                     off.ctypes.data))
    return out.reshape(-1, 2).T if ss else out


def _check_equal_widths(gr):
    """alignSignals' rule (R/zzzCountSignals.R:99-113): a sum over ranges needs ranges of one width."""
    w = np.asarray(gr.width)
    if w.size and np.any(w != w[0]):
        raise ValueError("all signals must have the same length")
    return int(w[0]) if w.size else 0


def _sum_shape(sums, ss):
    return sums.reshape(-1, 2).T.copy() if ss else sums


def pileup_sum(bampath, gr, tlen_filter, mapqual=0, binsize=1, shift=0, ss=False, requiredF=0,
               filteredF=-1, pe_mid=False, maxgap=16385, device=None):
    """bamProfile's signals summed over the ranges (bsig_pileup_sum): int64, ``(n_bins,)`` or ``(2, n_bins)``."""
    _check_gr(gr)
    w = _check_equal_widths(gr)
    head = _head(bampath, gr, tlen_filter)
    n_bins = (w + int(binsize) - 1) // int(binsize) if len(gr) and w > 0 else 0
    out = np.zeros(n_bins * (2 if ss else 1), dtype=np.int64)
    _lib.check(_lib.load().bsig_pileup_sum(*head, int(mapqual), int(binsize), int(shift), int(bool(ss)), int(requiredF),
                                           int(filteredF), int(bool(pe_mid)), int(maxgap), _dev(device), out.ctypes.data))
    return _sum_shape(out, ss)


def coverage_sum(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False,
                 maxgap=16385, device=None, *, binsize=1, ss=False, frag_len=0, spliced=False):
    """bamCoverage's signals summed over the ranges (bsig_coverage_sum): int64, ``(n_bins,)`` or ``(2, n_bins)``.
    ``frag_len`` (not with ``tspan``): of reads resized to the fragment (bsig_coverage_sum_resized).  ``spliced``: of the
    reads' aligned blocks (bsig_coverage_sum_spliced)."""
    _check_gr(gr)
    w = _check_equal_widths(gr)
    head = _head(bampath, gr, tlen_filter)
    n_bins = (w + int(binsize) - 1) // int(binsize) if len(gr) and w > 0 else 0
    out = np.zeros(n_bins * (2 if ss else 1), dtype=np.int64)
    fn, rule = _coverage_rule(_lib.load(), "sum", tspan, frag_len, spliced)
    _lib.check(fn(*head, int(mapqual), int(requiredF), int(filteredF), *rule, int(maxgap), _dev(device), int(binsize),
                  int(bool(ss)), out.ctypes.data))
    return _sum_shape(out, ss)


def _coverage_rule(lib, what, tspan, frag_len, spliced=False):
    """The file-level coverage call of a kind (``core_ex`` / ``sum`` / ``runs`` / ``views``) and the int32s that travel in its
    interval-rule slot: ``(tspan,)``, or with ``frag_len`` the resized call (bsig_coverage_<what>_resized) and the length, or
    with ``spliced`` the spliced call (bsig_coverage_<what>_spliced), which has no such slot."""
    base = "bsig_coverage_" + ("core" if what == "core_ex" else what)
    if spliced:
        if tspan or frag_len:
            raise ValueError("spliced coverage is of the reads' aligned blocks as they lie: no tspan, no frag_len")
        return getattr(lib, base + "_spliced"), ()
    if frag_len:
        if tspan:
            raise ValueError("a paired-end fragment already has its length: frag_len excludes tspan")
        return getattr(lib, base + "_resized"), (int(frag_len),)
    return getattr(lib, "bsig_coverage_" + what), (int(bool(tspan)),)


def pileup_xcorr(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, max_lag=500, maxgap=16385, device=None):
    """The strand cross-correlation over the ranges (bsig_pileup_xcorr): ``max_lag + 1 + 5`` int64, cross then moments."""
    head = _head(bampath, gr, tlen_filter)
    out = np.zeros(max(int(max_lag), 0) + 1 + _lib.XCORR_MOMENTS, dtype=np.int64)
    _lib.check(_lib.load().bsig_pileup_xcorr(*head, int(mapqual), int(requiredF), int(filteredF), int(max_lag), int(maxgap),
                                             _dev(device), out.ctypes.data))
    return out


def pileup_frag(bampath, gr, tlen_filter, mapqual=0, requiredF=66, filteredF=-1, pe_mid=False, len_bin=1, maxgap=16385,
                device=None):
    """The fragment-length histogram over the ranges (bsig_pileup_frag): ``tlen_filter[1] // len_bin + 1`` int64."""
    head = _head(bampath, gr, tlen_filter)
    tf = head.tf
    rows = int(tf[1]) // int(len_bin) + 1 if len(tf) == 2 and int(len_bin) >= 1 and tf[1] >= 0 else 1
    out = np.zeros(min(max(rows, 1), _lib.FRAG_MAX_ROWS), dtype=np.int64)
    _lib.check(_lib.load().bsig_pileup_frag(*head, int(mapqual), int(requiredF), int(filteredF), int(bool(pe_mid)), int(len_bin),
                                            int(maxgap), _dev(device), out.ctypes.data))
    return out


def pileup_vplot(bampath, gr, tlen_filter, mapqual=0, binsize=1, requiredF=66, filteredF=-1, pe_mid=False, len_bin=1,
                 maxgap=16385, device=None):
    """The V-plot over the ranges (bsig_pileup_vplot): ``(tlen_filter[1] // len_bin + 1, ceil(width / binsize))`` int64.
    The table's size is judged here, before a buffer is made; everything else by the library."""
    _check_gr(gr)
    w = _check_equal_widths(gr)
    head = _head(bampath, gr, tlen_filter)
    tf = head.tf
    ok = len(tf) == 2 and int(len_bin) >= 1 and int(binsize) >= 1 and tf[1] >= 0
    rows = int(tf[1]) // int(len_bin) + 1 if ok else 1
    cols = (w + int(binsize) - 1) // int(binsize) if ok and len(gr) and w > 0 else 0
    if rows > _lib.FRAG_MAX_ROWS or rows * cols > _lib.VPLOT_MAX_CELLS:
        rows, cols = 1, 0           # (the library refuses with its own sentence: nothing is written)
    out = np.zeros(max(rows * cols, 1), dtype=np.int64)
    _lib.check(_lib.load().bsig_pileup_vplot(*head, int(mapqual), int(binsize), int(requiredF), int(filteredF), int(bool(pe_mid)),
                                             int(len_bin), int(maxgap), _dev(device), out.ctypes.data))
    return out[:rows * cols].reshape(rows, cols)


def _hist_out(max_value):
    rows = min(max(int(max_value), 0), _lib.HIST_MAX_ROWS - 1) + 1
    return np.zeros(rows + _lib.HIST_MOMENTS, dtype=np.int64)


def pileup_hist(bampath, gr, tlen_filter, mapqual=0, ss=False, requiredF=0, filteredF=-1, pe_mid=False, max_value=1000,
                maxgap=16385, device=None):
    """The depth histogram of the 5' ends over the ranges (bsig_pileup_hist): ``max_value + 1 + 2`` int64, the histogram
    (last row: values >= ``max_value``) then the moments [cells, sum of the values]."""
    head = _head(bampath, gr, tlen_filter)
    out = _hist_out(max_value)
    _lib.check(_lib.load().bsig_pileup_hist(*head, int(mapqual), int(bool(ss)), int(requiredF), int(filteredF), int(bool(pe_mid)),
                                            int(max_value), int(maxgap), _dev(device), out.ctypes.data))
    return out


def coverage_hist(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False, max_value=1000,
                  maxgap=16385, device=None):
    """The depth histogram of the per-base coverage over the ranges (bsig_coverage_hist): as ``pileup_hist``."""
    head = _head(bampath, gr, tlen_filter)
    out = _hist_out(max_value)
    _lib.check(_lib.load().bsig_coverage_hist(*head, int(mapqual), int(requiredF), int(filteredF), int(bool(tspan)), int(max_value),
                                              int(maxgap), _dev(device), out.ctypes.data))
    return out


def _summary_call(fn, bampath, gr, tlen_filter, head, thresholds, rows, maxgap, device):
    """the two file-level summary calls: ``head`` = the int32 arguments between the length filter and the thresholds"""
    lead = _head(bampath, gr, tlen_filter)
    thr = np.ascontiguousarray([int(t) for t in thresholds], dtype=np.int32)
    k = min(len(thr), _lib.SUMMARY_MAX_THRESHOLDS)          # (more are refused by the call: the buffer need not hold them)
    out = np.zeros((len(gr), rows, _lib.SUMMARY_FIXED + k), dtype=np.int64)
    _lib.check(fn(*lead, *head, len(thr), thr.ctypes.data if len(thr) else None, int(maxgap), _dev(device), out.ctypes.data))
    return out


def pileup_summary(bampath, gr, tlen_filter, mapqual=0, ss=False, requiredF=0, filteredF=-1, pe_mid=False,
                   thresholds=(), maxgap=16385, device=None):
    """The per-range summaries of the 5' ends (bsig_pileup_summary): ``(n, S, 3 + K)`` int64 in the ranges' order, S = 2
    (sense, antisense) with ``ss``; a row is [sum, max, summit, cells >= thresholds[0], ...]."""
    head = (int(mapqual), int(bool(ss)), int(requiredF), int(filteredF), int(bool(pe_mid)))
    return _summary_call(_lib.load().bsig_pileup_summary, bampath, gr, tlen_filter, head, thresholds, 2 if ss else 1,
                         maxgap, device)


def coverage_summary(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False, thresholds=(),
                     maxgap=16385, device=None):
    """The per-range summaries of the per-base coverage (bsig_coverage_summary): ``(n, 1, 3 + K)`` int64, as
    ``pileup_summary``."""
    head = (int(mapqual), int(requiredF), int(filteredF), int(bool(tspan)))
    return _summary_call(_lib.load().bsig_coverage_summary, bampath, gr, tlen_filter, head, thresholds, 1, maxgap, device)


def _scaled_call(fn, bampath, gr, tlen_filter, head, n_bins, rows, maxgap, device):
    """the two file-level scaled-region calls: ``head`` = the int32 arguments between the length filter and n_bins"""
    lead = _head(bampath, gr, tlen_filter)
    n_bins = int(n_bins)
    # (a number of bins the call refuses: the buffer need not hold them)
    out = np.zeros((len(gr), rows, n_bins if 1 <= n_bins <= _lib.SCALED_MAX_BINS else 1), dtype=np.int64)
    _lib.check(fn(*lead, *head, n_bins, int(maxgap), _dev(device), out.ctypes.data))
    return out


def pileup_scaled(bampath, gr, tlen_filter, mapqual=0, ss=False, requiredF=0, filteredF=-1, pe_mid=False,
                  n_bins=100, maxgap=16385, device=None):
    """The scaled regions of the 5' ends (bsig_pileup_scaled): ``(n, S, n_bins)`` int64 in the ranges' order, S = 2
    (sense, antisense) with ``ss``; bin ``c * n_bins // w`` holds cell ``c`` of a range of width ``w``."""
    head = (int(mapqual), int(bool(ss)), int(requiredF), int(filteredF), int(bool(pe_mid)))
    return _scaled_call(_lib.load().bsig_pileup_scaled, bampath, gr, tlen_filter, head, n_bins, 2 if ss else 1, maxgap, device)


def coverage_scaled(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False, n_bins=100,
                    maxgap=16385, device=None):
    """The scaled regions of the per-base coverage (bsig_coverage_scaled): ``(n, 1, n_bins)`` int64, as
    ``pileup_scaled``."""
    head = (int(mapqual), int(requiredF), int(filteredF), int(bool(tspan)))
    return _scaled_call(_lib.load().bsig_coverage_scaled, bampath, gr, tlen_filter, head, n_bins, 1, maxgap, device)


def pileup_capped(bampath, gr, tlen_filter, mapqual=0, binsize=1, shift=0, ss=False, requiredF=0,
                  filteredF=-1, pe_mid=False, keep_dup=1, maxgap=16385, device=None):
    """``pileup_core`` with every per-base, per-strand 5'-end cell capped at ``keep_dup`` before it is binned or the
    strands are added (bsig_pileup_capped); the same list."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    n = len(gr)
    off = np.empty(n + 1, dtype=np.int64)
    cells = lib.bsig_layout(n, head.width.ctypes.data, int(binsize), int(bool(ss)), off.ctypes.data)
    out = np.zeros(cells, dtype=np.int32)
    _lib.check(lib.bsig_pileup_capped(*head, int(mapqual), int(binsize), int(shift), int(bool(ss)), int(requiredF),
                                      int(filteredF), int(bool(pe_mid)), int(keep_dup), int(maxgap), _dev(device),
                                      out.ctypes.data, off.ctypes.data))
    if binsize <= 0:
        return [out.reshape(-1, 2).T if ss else out]
    return _split(out, off, ss)


def coverage_capped(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False, frag_len=0, keep_dup=1,
                    maxgap=16385, device=None, *, binsize=1, ss=False):
    """``coverage_core(frag_len=)`` of the reads that ``keep_dup`` keeps: at most that many per 5' end and strand
    (bsig_coverage_capped); the same list."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    n = len(gr)
    off = np.empty(n + 1, dtype=np.int64)
    cells = lib.bsig_layout(n, head.width.ctypes.data, int(binsize), int(bool(ss)), off.ctypes.data)
    out = np.zeros(cells, dtype=np.int32)
    _lib.check(lib.bsig_coverage_capped(*head, int(mapqual), int(requiredF), int(filteredF), int(bool(tspan)), int(frag_len),
                                        int(keep_dup), int(maxgap), _dev(device), int(binsize), int(bool(ss)),
                                        out.ctypes.data, off.ctypes.data))
    return _split(out, off, bool(ss))


def _take_runs(lib, handle, ss):
    """a bsig_runs_result handle -> RunSignals (the arrays are allocated once the handle says how large they are)"""
    try:
        n_seg, n_runs = int(lib.bsig_runs_result_n_seg(handle)), int(lib.bsig_runs_result_n_runs(handle))
        seg_off = np.empty(n_seg + 1, dtype=np.int64)
        values = np.empty(n_runs, dtype=np.int32)
        lengths = np.empty(n_runs, dtype=np.int32)
        _lib.check(lib.bsig_runs_result_copy(handle, seg_off.ctypes.data, values.ctypes.data, lengths.ctypes.data))
    finally:
        lib.bsig_runs_result_free(handle)
    return RunSignals(seg_off, values, lengths, bool(ss))


def pileup_runs(bampath, gr, tlen_filter, mapqual=0, binsize=1, shift=0, ss=False, requiredF=0,
                filteredF=-1, pe_mid=False, maxgap=16385, device=None):
    """bamProfile's signals as runs (bsig_pileup_runs): a RunSignals; the per-base cells stay on the GPU."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.bsig_pileup_runs(*head, int(mapqual), int(binsize), int(shift), int(bool(ss)), int(requiredF), int(filteredF),
                                    int(bool(pe_mid)), int(maxgap), _dev(device), C.byref(h)))
    return _take_runs(lib, h, ss)


def coverage_runs(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False,
                  maxgap=16385, device=None, *, binsize=1, ss=False, frag_len=0, spliced=False):
    """bamCoverage's signals as runs (bsig_coverage_runs): a RunSignals; the per-base cells stay on the GPU.
    ``frag_len`` (not with ``tspan``): of reads resized to the fragment (bsig_coverage_runs_resized).  ``spliced``: of the
    reads' aligned blocks (bsig_coverage_runs_spliced)."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    h = C.c_void_p()
    fn, rule = _coverage_rule(lib, "runs", tspan, frag_len, spliced)
    _lib.check(fn(*head, int(mapqual), int(requiredF), int(filteredF), *rule, int(maxgap), _dev(device), int(binsize),
                  int(bool(ss)), C.byref(h)))
    return _take_runs(lib, h, ss)


def _take_views(lib, handle, ss):
    """a bsig_views_result handle -> SignalViews (the arrays are allocated once the handle says how large they are)"""
    from .views import SignalViews
    try:
        n_seg, n = int(lib.bsig_views_result_n_seg(handle)), int(lib.bsig_views_result_n_views(handle))
        out = [np.empty(n_seg + 1, dtype=np.int64)] + [np.empty(n, dtype=dt) for dt in (np.int32, np.int32, np.int64, np.int32, np.int32)]
        _lib.check(lib.bsig_views_result_copy(handle, *[a.ctypes.data if a.size else None for a in out]))
    finally:
        lib.bsig_views_result_free(handle)
    return SignalViews(*out, bool(ss))


def pileup_views(bampath, gr, tlen_filter, lower, upper, mapqual=0, binsize=1, shift=0, ss=False, requiredF=0,
                 filteredF=-1, pe_mid=False, maxgap=16385, device=None):
    """The views of bamProfile's signals (bsig_pileup_views): a SignalViews of the stretches with ``lower <= v <= upper``;
    the per-base cells stay on the GPU."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.bsig_pileup_views(*head, int(mapqual), int(binsize), int(shift), int(bool(ss)), int(requiredF), int(filteredF),
                                     int(bool(pe_mid)), int(maxgap), _dev(device), int(lower), int(upper), C.byref(h)))
    return _take_views(lib, h, ss)


def coverage_views(bampath, gr, tlen_filter, lower, upper, mapqual=0, requiredF=0, filteredF=-1, tspan=False,
                   maxgap=16385, device=None, *, binsize=1, ss=False, frag_len=0, spliced=False):
    """The views of bamCoverage's signals (bsig_coverage_views): a SignalViews, as ``pileup_views``.
    ``frag_len`` (not with ``tspan``): of reads resized to the fragment (bsig_coverage_views_resized).  ``spliced``: of the
    reads' aligned blocks (bsig_coverage_views_spliced)."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    h = C.c_void_p()
    fn, rule = _coverage_rule(lib, "views", tspan, frag_len, spliced)
    _lib.check(fn(*head, int(mapqual), int(requiredF), int(filteredF), *rule, int(maxgap), _dev(device), int(binsize),
                  int(bool(ss)), int(lower), int(upper), C.byref(h)))
    return _take_views(lib, h, ss)


def _is_ex(binsize, ss):
    """bins or strands take bsig_coverage_core_ex[_into]; the defaults keep the reference's own entry point"""
    return int(binsize) != 1 or bool(ss)


def coverage_core(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False,
                  maxgap=16385, device=None, *, binsize=1, ss=False, frag_len=0, spliced=False):
    """The native entry point behind bamCoverage (ref: R/RcppExports.R:16-18).  ``binsize`` / ``ss``:
    per-base coverage summed over bins / split into sense and antisense rows (bsig_coverage_core_ex).
    ``frag_len`` (not with ``tspan``): of reads resized to the fragment (bsig_coverage_core_resized, whatever the bins).
    ``spliced``: of the reads' aligned blocks (bsig_coverage_core_spliced, whatever the bins)."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    n = len(gr)
    ex = _is_ex(binsize, ss) or bool(frag_len) or bool(spliced)
    off = np.empty(n + 1, dtype=np.int64)
    cells = lib.bsig_layout(n, head.width.ctypes.data, int(binsize) if ex else 1, int(bool(ss)) if ex else 0, off.ctypes.data)
    out = np.zeros(cells, dtype=np.int32)
    flt = (int(mapqual), int(requiredF), int(filteredF))
    if ex:
        fn, rule = _coverage_rule(lib, "core_ex", tspan, frag_len, spliced)
        _lib.check(fn(*head, *flt, *rule, int(maxgap), _dev(device), int(binsize), int(bool(ss)), out.ctypes.data, off.ctypes.data))
    else:
        _lib.check(lib.bsig_coverage_core(*head, *flt, int(bool(tspan)), int(maxgap), _dev(device), out.ctypes.data, off.ctypes.data))
    return _split(out, off, ex and bool(ss))


def _alloc_signals(width, binsize, ss):
    """allocateList (ref: src/bamsignals.cpp:139-192): the per-range vectors / 2 x w matrices, made before the
    counting; returns (list as the caller sees it, the arrays the native side writes into)."""
    mult = 2 if ss else 1
    if binsize <= 0:
        v = np.empty(len(width) * mult, dtype=np.int32)
        return [v.reshape(-1, 2).T if ss else v], [v]
    cells = [0 if w <= 0 else mult * ((int(w) + binsize - 1) // binsize) for w in width]
    vs = [np.empty(c, dtype=np.int32) for c in cells]
    return [v.reshape(-1, 2).T if ss else v for v in vs], vs


def _dest_pointers(vs):
    return (C.c_void_p * max(len(vs), 1))(*[v.ctypes.data if v.size else None for v in vs])


def pileup_core_into(bampath, gr, tlen_filter, mapqual=0, binsize=1, shift=0, ss=False, requiredF=0,
                     filteredF=-1, pe_mid=False, maxgap=16385, device=None):
    """pileup_core with the result delivered in place (bsig_pileup_core_into, what the R shim binds): the
    per-range arrays are allocated first, as allocateList does, and the native side writes straight into them."""
    head = _head(bampath, gr, tlen_filter)
    out, vs = _alloc_signals(head.width, int(binsize), bool(ss))
    _lib.check(_lib.load().bsig_pileup_core_into(*head, int(mapqual), int(binsize), int(shift), int(bool(ss)), int(requiredF),
                                                 int(filteredF), int(bool(pe_mid)), int(maxgap), _dev(device), _dest_pointers(vs)))
    return out


def coverage_core_into(bampath, gr, tlen_filter, mapqual=0, requiredF=0, filteredF=-1, tspan=False,
                       maxgap=16385, device=None, *, binsize=1, ss=False):
    """coverage_core with the result delivered in place (bsig_coverage_core_into / bsig_coverage_core_ex_into)."""
    head = _head(bampath, gr, tlen_filter)
    lib = _lib.load()
    ex = _is_ex(binsize, ss)
    out, vs = _alloc_signals(head.width, max(int(binsize), 1) if ex else 1, ex and bool(ss))
    rest = (int(mapqual), int(requiredF), int(filteredF), int(bool(tspan)), int(maxgap), _dev(device))
    if ex:
        _lib.check(lib.bsig_coverage_core_ex_into(*head, *rest, int(binsize), int(bool(ss)), _dest_pointers(vs)))
    else:
        _lib.check(lib.bsig_coverage_core_into(*head, *rest, _dest_pointers(vs)))
    return out


def last_call_timing():
    """Stage seconds of this thread's last bamCount/bamProfile/bamCoverage call, and where the stages' time went
    (``alloc_*``: seconds inside the driver's allocator -- hipMalloc, hipFree, hipHostMalloc -- metered per
    process; ``plan`` / ``kernels`` / ``download``: the parts of ``plan_run_download`` on one GPU)."""
    t = (C.c_double * 16)()
    _lib.load().bsig_last_call_timing_ex(t, 16)
    return dict(open=t[0], decode=t[1], upload_and_layout=t[2], plan_run_download=t[3], total=t[4],
                bam_was_resident=bool(t[5]), alloc_in_decode_and_layout=t[6], alloc_in_plan_run_download=t[7],
                alloc_total=t[8], plan=t[9], kernels=t[10], download=t[11], alloc_calls=int(t[12]),
                reserved_bytes=int(t[14]), reservation_wait=t[15])


def last_call_route():
    """How this thread's last file-level call was carried out (GPUs, decode route, result route)."""
    return _lib.load().bsig_last_call_route().decode()


def _keep_dup(keepDup, paired_end, choices):  # noqa: N803
    """keepDup as a call reads it: 0 for None, else a whole number in 1 .. 2**31 - 1, and only for single ends"""
    if keepDup is None:
        return 0
    if isinstance(keepDup, (bool, np.bool_)) or not isinstance(keepDup, (int, float, np.integer, np.floating)) \
            or not float(keepDup).is_integer():
        raise ValueError("keepDup must be a whole number of reads")
    k = int(keepDup)
    if k < 1:
        raise ValueError("keepDup must be at least 1")
    if k > _lib.KEEP_DUP_MAX:
        raise ValueError(f"keepDup must be at most {_lib.KEEP_DUP_MAX}")
    if _match_arg(paired_end, choices, "paired.end") != "ignore":
        raise ValueError('keepDup caps single-end reads by their 5\' end and strand: a paired-end duplicate is a fragment with '
                         'both ends equal, which those do not identify (paired_end must be "ignore")')
    return k


def bamCount(bampath, gr, mapqual=0, shift=0, ss=False, paired_end=("ignore", "filter", "midpoint"),  # noqa: N802
             tlenFilter=None, filteredFlag=-1, verbose=True, *, keepDup=None):  # noqa: N803
    """For each range, count the reads whose 5' end maps in it (R/wrappers.R:101-120).
    Returns an int32 vector, or a 2 x n matrix (rows sense, antisense) with ``ss=True``.

    ``keepDup=k`` (keyword only; a whole number in 1 .. 2**31 - 1; ``None``, the default: every read counts): at most ``k``
    reads per position and strand, MACS's ``--keep-dup k``.  Of the reads that pass the filter, ``e_s[p]`` have their 5' end
    -- ``pos`` of a forward read, ``end`` of a reverse one, after ``shift`` -- on base ``p`` and strand ``s``; a range's
    count is the sum of ``min(e_s[p], k)`` over its bases, per strand with ``ss`` and over both strands without (the cap
    is applied per strand first).  ``paired_end`` must be ``"ignore"``."""
    k = _keep_dup(keepDup, paired_end, ("ignore", "filter", "midpoint"))
    if verbose:
        _print_sentence(bampath)
    pe = _match_arg(paired_end, ("ignore", "filter", "midpoint"), "paired.end")
    if k:
        return pileup_capped(os.path.expanduser(str(bampath)), gr, (), mapqual, -1, shift, ss, flagMask(pe), filteredFlag,
                             False, k)[0]
    pu = pileup_core(os.path.expanduser(str(bampath)), gr, globals()["tlenFilter"](tlenFilter, pe), mapqual, -1,
                     shift, ss, flagMask(pe), filteredFlag, pe == "midpoint")
    return pu[0]


def bamProfile(bampath, gr, binsize=1, mapqual=0, shift=0, ss=False,  # noqa: N802
               paired_end=("ignore", "filter", "midpoint"), tlenFilter=None, filteredFlag=-1, verbose=True,  # noqa: N803
               *, aggregate=False, runs=False, keepDup=None):
    """For each base pair (or bin) of the ranges, the number of reads whose 5' end maps there
    (R/wrappers.R:124-151).  Returns a CountSignals.

    ``aggregate=True``: ranges of one width only; returns the int64 sum over the ranges of their signals, cell by
    cell -- ``np.asarray(sig.alignSignals(), np.int64).sum(axis=-1)`` of the CountSignals above, shape ``(n_bins,)``
    or ``(2, n_bins)`` with ``ss`` -- computed on the GPU without the per-range result.  The metaprofile (the
    vignette's rowMeans of alignSignals) is this divided by ``len(gr)``.

    ``runs=True``: returns a RunSignals -- the same signals as runs (value, length), encoded on the GPU, so that the
    per-base cells are never downloaded; ``sig.decode(i)`` is the CountSignals' element i.  Not with ``aggregate``.

    ``keepDup=k`` (a whole number in 1 .. 2**31 - 1; ``None``, the default: every read counts): at most ``k`` reads per
    position and strand, MACS's ``--keep-dup k``.  Of the reads that pass the filter, ``e_s[p]`` have their 5' end -- ``pos``
    of a forward read, ``end`` of a reverse one, after ``shift`` -- on base ``p`` and strand ``s``; bin j of a range holds
    the sum of ``min(e_s[p], k)`` over the bin's bases, sense and antisense as separate rows with ``ss`` and added
    without (the cap is applied per strand first; a '-' range is mirrored first and binned second, and its strands swap,
    as always).  The reads that share a cell are indistinguishable, so which of them survive never matters.
    ``paired_end`` must be ``"ignore"``; not with ``aggregate`` or ``runs`` (not built yet)."""
    if runs and aggregate:
        raise ValueError("runs=True and aggregate=True exclude each other: a sum over ranges has no per-range runs")
    k = _keep_dup(keepDup, paired_end, ("ignore", "filter", "midpoint"))
    if k and (aggregate or runs):
        raise ValueError("keepDup with aggregate=True or runs=True is out of scope so far: take the per-range signals")
    if verbose:
        _print_sentence(bampath)
    if binsize < 1:
        raise ValueError("provide a binsize greater or equal to 1")
    _check_gr(gr)
    if aggregate:
        _check_equal_widths(gr)
    if binsize > 1 and np.any(gr.width % binsize != 0):
        warnings.warn("some ranges' widths are not a multiple of the selected\n"
                      "             binsize, some bins will correspond to less than binsize basepairs")
    pe = _match_arg(paired_end, ("ignore", "filter", "midpoint"), "paired.end")
    if aggregate:
        return pileup_sum(os.path.expanduser(str(bampath)), gr, globals()["tlenFilter"](tlenFilter, pe), mapqual,
                          int(binsize), shift, ss, flagMask(pe), filteredFlag, pe == "midpoint")
    if runs:
        return pileup_runs(os.path.expanduser(str(bampath)), gr, globals()["tlenFilter"](tlenFilter, pe), mapqual,
                           int(binsize), shift, ss, flagMask(pe), filteredFlag, pe == "midpoint")
    if k:
        pu = pileup_capped(os.path.expanduser(str(bampath)), gr, (), mapqual, int(binsize), shift, ss, flagMask(pe),
                           filteredFlag, False, k)
        return CountSignals(pu, bool(ss), _trusted=True)
    pu = pileup_core(os.path.expanduser(str(bampath)), gr, globals()["tlenFilter"](tlenFilter, pe), mapqual,
                     int(binsize), shift, ss, flagMask(pe), filteredFlag, pe == "midpoint")
    return CountSignals(pu, bool(ss), _trusted=True)


# widest coverage bin (include/bamsignals_abi.h, BSIG_MODE_COVERAGE_EX): a tile's sums cannot wrap below it
MAX_COVERAGE_BINSIZE = 65536


def _coverage_binsize(binsize):
    if isinstance(binsize, (bool, np.bool_)) or not isinstance(binsize, (int, float, np.integer, np.floating)) \
            or not float(binsize).is_integer():
        raise ValueError("binsize must be a whole number of bases")
    b = int(binsize)
    if b < 1:
        raise ValueError("provide a binsize greater or equal to 1")
    if b > MAX_COVERAGE_BINSIZE:
        raise ValueError(f"coverage bins are at most {MAX_COVERAGE_BINSIZE} bases wide; count at that scale with "
                         "bamProfile or bamCount")
    return b


# longest fragment reads are resized to (include/bamsignals_abi.h, BSIG_FRAG_LEN_MAX)
MAX_FRAG_LENGTH = 1 << 24


def _frag_length(fragLength):  # noqa: N803
    if fragLength is None:
        return 0
    if isinstance(fragLength, (bool, np.bool_)) or not isinstance(fragLength, (int, float, np.integer, np.floating)) \
            or not float(fragLength).is_integer():
        raise ValueError("fragLength must be a whole number of bases")
    f = int(fragLength)
    if f < 1:
        raise ValueError("fragLength must be at least 1")
    if f > MAX_FRAG_LENGTH:
        raise ValueError(f"fragLength must be at most {MAX_FRAG_LENGTH}")
    return f


def _splice(splice, paired_end, choices, fragLength=None, keepDup=None):  # noqa: N803
    """splice as a call reads it: a bool, and only for the reads as they lie"""
    if not isinstance(splice, (bool, np.bool_)):
        raise ValueError("splice must be True or False")
    if not splice:
        return False
    if fragLength is not None:
        raise ValueError("splice with fragLength: every aligned block of a read would be resized, not the read")
    if keepDup is not None:
        raise ValueError("splice with keepDup: reads are capped by their 5' end, and a block's start is not one")
    if _match_arg(paired_end, choices, "paired.end") != "ignore":
        raise ValueError('splice with paired_end="extend": every aligned block of a read would be extended to the whole '
                         'fragment, introns included (paired_end must be "ignore")')
    return True


def bamCoverage(bampath, gr, mapqual=0, paired_end=("ignore", "extend"), tlenFilter=None,  # noqa: N802,N803
                filteredFlag=-1, verbose=True, *, binsize=1, ss=False, aggregate=False, runs=False, fragLength=None,
                keepDup=None, splice=False):
    """For each base pair of the ranges, the number of reads covering it (R/wrappers.R:154-173).

    ``binsize`` (1 .. 65,536): bin j of a range covers its bases [j*binsize, min((j+1)*binsize, width)) in range
    orientation (a '-' range is mirrored first and binned second, as in bamProfile) and holds the sum of the per-base
    coverage over them, so ``bamCoverage(binsize=b)[i] == np.add.reduceat(bamCoverage()[i], np.arange(0, w_i, b))``;
    the last bin of a range may be shorter (warned about, as bamProfile does).
    ``ss=True``: each signal is a 2 x n_bins matrix, row 0 (sense) the coverage by reads on the range's strand
    ('*' counts as '+'), row 1 (antisense) by the others; with ``paired_end="extend"`` the whole fragment counts on
    the strand of the read that passed the flag mask (the first mate).  sense + antisense is the unstranded result.
    A bin whose sum would exceed 2^31 - 1 raises BsigError.  The defaults are the reference's call.
    ``aggregate=True``: the int64 sum over ranges of one width, as in ``bamProfile``.
    ``runs=True``: a RunSignals instead of a CountSignals, as in ``bamProfile`` -- the form of an RleList or a bedGraph
    (``sig.to_bedgraph``); a whole-genome track without its 4 bytes per base in host memory.  Not with ``aggregate``.
    ``fragLength=L`` (a whole number in 1 .. 2**24; ``None``: the read as it lies): single-end reads resized to the
    fragment, the signal of MACS ``--extsize``, deepTools ``--extendReads N``, csaw ``ext`` and
    ``coverage(resize(reads, L, fix="start"))``.  A read that passes the filter covers exactly ``L`` bases from its 5' end
    in its own direction: forward (flag & 16 == 0) ``[pos, pos + L - 1]``, reverse ``[end - L + 1, end]``, ``pos`` and
    ``end`` its first and last aligned base.  ``L`` below the read's length trims it, ``L = 1`` is its 5' end.  Nothing
    is clipped at the reference's last base (a range that overhangs it sees the overhang of a forward fragment); bases
    below 0 exist in no range.  With ``ss`` the fragment counts on the read's own strand; ``binsize``, ``aggregate``
    and ``runs`` work on it as on plain coverage.  ``paired_end`` must be ``"ignore"``: a paired-end fragment already
    has its length (``"extend"``).  The length comes from the data:
    ``fragLength=bamCrossCorr(...).fragment_length()``.
    ``keepDup=k`` (a whole number in 1 .. 2**31 - 1; ``None``, the default: every read counts), with ``fragLength=L`` only:
    at most ``k`` reads per position and strand, MACS's ``--keep-dup k`` beside its ``--extsize``.  Of the reads that pass
    the filter, ``e_s[p]`` have their 5' end on base ``p`` and strand ``s``; with ``c_s[p] = min(e_s[p], k)`` every kept
    read covers ``L`` bases from its 5' end in its own direction, so in range orientation cell ``x`` is the sum of
    ``c_sense[p]`` over ``p = x - L + 1 .. x`` plus the sum of ``c_anti[p]`` over ``p = x .. x + L - 1``, 5' ends up to
    ``L - 1`` bases outside the range included; with ``ss`` the two sums are the two rows, and ``binsize`` sums cells as
    for plain coverage.  Without ``fragLength`` it is refused: duplicates of different lengths have no defined survivor.
    ``paired_end`` must be ``"ignore"``; not with ``aggregate`` or ``runs`` (not built yet).
    ``splice=True`` (a bool; ``False``, the default, is the reference's call): coverage that skips the reads' ``N`` gaps, as
    ``GenomicAlignments::coverage()``, deepTools ``bamCoverage`` and ``bedtools genomecov -split`` do -- what RNA-seq needs,
    where a read ``40M2000N60M`` otherwise fills its intron.  Walk the CIGAR from ``pos``: ``M D = X`` advance and are
    covered, ``N`` advances and is not, ``I S H P`` advance nothing; a read covers its aligned blocks, the stretches between
    its gaps (neighbouring ``N``, and ``N`` separated only by ``I S H P``, are one gap; ``D`` stays covered).  ``mapqual``
    and ``filteredFlag`` act on a read's blocks as on the read.  ``binsize``, ``ss``, ``aggregate`` and ``runs`` work on it
    as on plain coverage; ``bamCoverage(splice=True) <= bamCoverage()`` cell by cell, and on a file without ``N`` they are
    equal.  Not with ``paired_end="extend"``, ``fragLength`` or ``keepDup``.  The file's spliced reads are a resident set of
    their own beside its plain ones."""
    if runs and aggregate:
        raise ValueError("runs=True and aggregate=True exclude each other: a sum over ranges has no per-range runs")
    sp = _splice(splice, paired_end, ("ignore", "extend"), fragLength, keepDup)
    k = _keep_dup(keepDup, paired_end, ("ignore", "extend"))
    if k and fragLength is None:
        raise ValueError("keepDup needs fragLength for bamCoverage: duplicates of different lengths have no defined survivor")
    if k and (aggregate or runs):
        raise ValueError("keepDup with aggregate=True or runs=True is out of scope so far: take the per-range signals")
    frag = _frag_length(fragLength)
    if frag and _match_arg(paired_end, ("ignore", "extend"), "paired.end") != "ignore":
        raise ValueError('fragLength resizes single-end reads: with paired_end="extend" a fragment already has its length, '
                         "its template length (use one or the other)")
    if verbose:
        _print_sentence(bampath)
    b = _coverage_binsize(binsize)
    _check_gr(gr)
    if aggregate:
        _check_equal_widths(gr)
    if b > 1 and np.any(gr.width % b != 0):
        warnings.warn("some ranges' widths are not a multiple of the selected\n"
                      "             binsize, some bins will correspond to less than binsize basepairs")
    pe = _match_arg(paired_end, ("ignore", "extend"), "paired.end")
    sp_kw = dict(spliced=True) if sp else {}        # (the plain calls stay exactly the calls they were)
    if aggregate:
        return coverage_sum(os.path.expanduser(str(bampath)), gr, globals()["tlenFilter"](tlenFilter, pe), mapqual,
                            flagMask(pe), filteredFlag, pe == "extend", binsize=b, ss=bool(ss), frag_len=frag, **sp_kw)
    if runs:
        return coverage_runs(os.path.expanduser(str(bampath)), gr, globals()["tlenFilter"](tlenFilter, pe), mapqual,
                             flagMask(pe), filteredFlag, pe == "extend", binsize=b, ss=bool(ss), frag_len=frag, **sp_kw)
    if k:
        pu = coverage_capped(os.path.expanduser(str(bampath)), gr, (), mapqual, flagMask(pe), filteredFlag, False, frag, k,
                             binsize=b, ss=bool(ss))
        return CountSignals(pu, bool(ss), _trusted=True)
    pu = coverage_core(os.path.expanduser(str(bampath)), gr, globals()["tlenFilter"](tlenFilter, pe), mapqual,
                       flagMask(pe), filteredFlag, pe == "extend", binsize=b, ss=bool(ss), frag_len=frag, **sp_kw)
    return CountSignals(pu, bool(ss), _trusted=True)
