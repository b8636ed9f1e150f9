"""bamVPlot: fragment length by position over ranges of one width -- the V-plot.

Paired-end reads carry two facts about a fragment: where it lies and how long it is.  ``bamFragSizes`` gives the length
histogram summed over all positions, ``bamProfile(..., paired_end="midpoint", aggregate=True)`` the midpoint profile
summed over all lengths; their joint table is the V-plot (Henikoff's V-plots, ATACseqQC ``vPlot``, NucleoATAC's input,
plot2DO): row = fragment length, column = the fragment's midpoint (or 5' end) relative to the range, summed over ranges
of one width -- TSSs, motif sites, nucleosome dyads.  It shows nucleosome-free fragments piling on the site and
mono-nucleosomes phasing beside it; neither marginal holds that.  The table is made on the GPU in one pass over the reads
(bsig_pileup_vplot); only its cells come back.
"""
from __future__ import annotations

import os
import warnings

import numpy as np

from . import _lib
from . import wrappers as _w
from .fragsizes import FragSizes, _lenbin

# include/bamsignals_abi.h: BSIG_FRAG_MAX_ROWS, BSIG_VPLOT_MAX_CELLS
MAX_ROWS = _lib.FRAG_MAX_ROWS
MAX_CELLS = _lib.VPLOT_MAX_CELLS


class VPlot:
    """The integers of a V-plot, read-only.

    ``counts[r, j]`` (int64): the fragments with ``|tlen| // lenbin == r`` whose position lies in column j of a range,
    summed over the ranges.  ``lengths[r] = r * lenbin``: the first length of row r; ``positions[j] = j * binsize``: the
    first range-relative base (0-based, in the range's own orientation) of column j.  ``n``: the total."""

    __slots__ = ("_counts", "_lenbin", "_binsize", "_lengths", "_positions", "_n")

    def __init__(self, counts, lenbin=1, binsize=1):
        c = np.array(counts, dtype=np.int64)
        if c.ndim != 2:
            raise ValueError("counts must be a 2-D table (lengths x positions)")
        c.setflags(write=False)
        lb = _lenbin(lenbin)
        bs = _binsize(binsize)
        lengths = np.arange(c.shape[0], dtype=np.int64) * lb
        positions = np.arange(c.shape[1], dtype=np.int64) * bs
        lengths.setflags(write=False)
        positions.setflags(write=False)
        object.__setattr__(self, "_counts", c)
        object.__setattr__(self, "_lenbin", lb)
        object.__setattr__(self, "_binsize", bs)
        object.__setattr__(self, "_lengths", lengths)
        object.__setattr__(self, "_positions", positions)
        object.__setattr__(self, "_n", int(c.sum(dtype=object)) if c.size else 0)       # (exact past int64)

    def __setattr__(self, name, value):
        raise AttributeError("VPlot is read-only")

    counts = property(lambda self: self._counts)
    lenbin = property(lambda self: self._lenbin)
    binsize = property(lambda self: self._binsize)
    lengths = property(lambda self: self._lengths)
    positions = property(lambda self: self._positions)
    n = property(lambda self: self._n)

    def frag_sizes(self):
        """The row sums as a ``FragSizes``: what ``bamFragSizes`` returns for the same arguments."""
        return FragSizes(self._counts.sum(axis=1, dtype=np.int64), self._lenbin)

    def profile(self):
        """The column sums (int64): what ``bamProfile(..., aggregate=True)`` returns for the same arguments."""
        return self._counts.sum(axis=0, dtype=np.int64)

    def band(self, lo, hi):
        """The profile of the fragments of lengths ``lo .. hi`` (int64, one cell per column).  ``lo`` must be a row's
        first length and ``hi`` a row's last (``band(0, 99)`` against ``band(180, 249)``: nucleosome-free against
        mono-nucleosome); anything else is a ValueError, never a silently rounded band."""
        lo, hi = int(lo), int(hi)
        lb, rows = self._lenbin, self._counts.shape[0]
        if lo < 0 or lo % lb != 0:
            raise ValueError(f"lo = {lo} is not the first length of a row (rows are {lb} lengths wide)")
        if hi < lo or (hi + 1) % lb != 0:
            raise ValueError(f"hi = {hi} is not the last length of a row at or above lo (rows are {lb} lengths wide)")
        if (hi + 1) // lb > rows:
            raise ValueError(f"hi = {hi} lies beyond the last row ({rows * lb - 1})")
        return self._counts[lo // lb:(hi + 1) // lb].sum(axis=0, dtype=np.int64)

    def __repr__(self):
        return (f"VPlot(rows={self._counts.shape[0]}, cols={self._counts.shape[1]}, lenbin={self._lenbin}, "
                f"binsize={self._binsize}, n={self._n})")


def _binsize(binsize):
    if isinstance(binsize, (bool, np.bool_)) or not isinstance(binsize, (int, float, np.integer, np.floating)) \
            or not float(binsize).is_integer():
        raise ValueError("binsize must be a whole number of bases")
    b = int(binsize)
    if b < 1:
        raise ValueError("provide a binsize greater or equal to 1")
    return b


def bamVPlot(bampath, gr, tlenFilter=None, lenbin=1, binsize=1, paired_end=("midpoint", "filter"), mapqual=0,  # noqa: N802,N803
             filteredFlag=-1, verbose=True):
    """The V-plot over the ranges ``gr``, all of one width w: ``tlenFilter[1] // lenbin + 1`` rows (``tlenFilter`` None:
    (0, 1000); at most ``MAX_ROWS``) by ``ceil(w / binsize)`` columns (at most ``MAX_CELLS`` cells).

    ``counts[r, j]`` is the sum over the ranges of cell j of ``bamProfile(bampath, gr[i], binsize=binsize,
    paired_end=paired_end, tlenFilter=row r's lengths)``: a fragment counts through the first read of its proper pair,
    at its midpoint ("midpoint", the default) or its 5' end ("filter"), once per range that holds that position; a '-'
    range is mirrored first and binned second.  ``mapqual`` and ``filteredFlag`` filter the reads as in ``bamProfile``.
    Returns a ``VPlot``: ``vp.frag_sizes()`` is ``bamFragSizes`` and ``vp.profile()`` is ``bamProfile(...,
    aggregate=True)`` with the same arguments."""
    if verbose:
        _w._print_sentence(bampath)
    lb = _lenbin(lenbin)
    bs = _binsize(binsize)
    _w._check_gr(gr)
    w = _w._check_equal_widths(gr)
    if bs > 1 and np.any(np.asarray(gr.width) % bs != 0):
        warnings.warn("some ranges' widths are not a multiple of the selected\n"
                      "             binsize, some bins will correspond to less than binsize basepairs")
    pe = _w._match_arg(paired_end, ("midpoint", "filter"), "paired.end")
    tf = _w.tlenFilter(tlenFilter, pe)
    rows = tf[1] // lb + 1
    cols = (w + bs - 1) // bs if len(gr) and w > 0 else 0
    if rows > MAX_ROWS:
        raise ValueError(f"tlenFilter[1] // lenbin + 1 = {rows} rows, at most {MAX_ROWS} fit: choose a wider lenbin")
    if rows * cols > MAX_CELLS:
        raise ValueError(f"{rows} rows x {cols} columns are more than {MAX_CELLS} cells: choose a wider lenbin or binsize")
    out = _w.pileup_vplot(os.path.expanduser(str(bampath)), gr, tf, mapqual, bs, _w.flagMask(pe), filteredFlag,
                          pe == "midpoint", lb)
    return VPlot(out, lb, bs)
