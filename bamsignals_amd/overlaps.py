"""bamOverlaps: for each range, the reads (or fragments) that overlap it.

bamCount counts the reads whose 5' end (or fragment midpoint) falls in a range, bamCoverage the reads over a base.  The
count most downstream tools start from is a third one -- countOverlaps / summarizeOverlaps, featureCounts, bedtools
multicov, csaw's regionCounts, DiffBind's count matrix: a read counts for a range when it shares bases with it.  A read that
starts 40 bases in front of a peak and reaches 60 bases into it counts here, and not for bamCount.  Counted on the GPU
(bsig_overlap_core); one int32 per range and strand comes back.
"""
from __future__ import annotations

import os

import numpy as np

from . import wrappers as _w


def _minoverlap(minoverlap):
    if isinstance(minoverlap, (bool, np.bool_)) or not isinstance(minoverlap, (int, float, np.integer, np.floating)) \
            or not float(minoverlap).is_integer():
        raise ValueError("minoverlap must be a whole number of bases")
    m = int(minoverlap)
    if m < 1:
        raise ValueError("minoverlap must be at least 1")
    if m > 2**31 - 1:
        raise ValueError("minoverlap must be below 2^31")
    return m


def bamOverlaps(bampath, gr, mapqual=0, type=("any", "within"), minoverlap=1, ss=False,  # noqa: N802,A002
                paired_end=("ignore", "filter", "extend"), tlenFilter=None, filteredFlag=-1, verbose=True):  # noqa: N803
    """For each range, count the reads that overlap it.

    A read that passes the filters (``mapqual``, ``filteredFlag``, and with ``paired_end`` other than "ignore" the first
    mate of a proper pair whose \\|tlen\\| lies in ``tlenFilter``, None: (0, 1000)) has the interval ``[s, e]`` = its first
    and last aligned base; with ``paired_end="extend"`` the whole fragment, as in ``bamCoverage``.  Against a range
    ``[lo, hi)`` it overlaps in ``ov = min(e, hi - 1) - max(s, lo) + 1`` bases.

    ``type="any"``: the read counts iff ``ov >= minoverlap``.  ``type="within"``: iff it also lies inside the range
    (``s >= lo`` and ``e <= hi - 1``).  Ranges may overlap or repeat -- each gets its own count -- and a zero-width range
    counts 0.  ``ss=True``: a counted read goes to the antisense row iff its strand differs from the range's ('*' counts as
    '+'); without ``ss`` the range's strand is not read.

    Returns what ``bamCount`` returns: an int32 vector, or a 2 x n matrix (rows sense, antisense) with ``ss=True``."""
    kind = _w._match_arg(type, ("any", "within"), "type")
    m = _minoverlap(minoverlap)
    pe = _w._match_arg(paired_end, ("ignore", "filter", "extend"), "paired.end")
    _w._check_gr(gr)
    tf = _w.tlenFilter(tlenFilter, pe)
    if verbose:
        _w._print_sentence(bampath)
    return _w.overlap_core(os.path.expanduser(str(bampath)), gr, tf, mapqual, kind == "within", m, bool(ss),
                           _w.flagMask(pe), filteredFlag, pe == "extend")
