"""bamScaled: every range cut into the same number of bins, whatever its width -- the scaled-region signal.

The heatmap matrix with one row per gene and ``nbins`` columns from TSS to TES, and the metaprofile over gene bodies,
peaks or capture targets of unequal width: cell ``c`` of a range of width ``w`` (the cells of ``bamCoverage`` /
``bamProfile``, a '-' range mirrored) belongs to bin ``c * nbins // w``.  The bins are summed on the GPU
(bsig_coverage_scaled / bsig_pileup_scaled), where the per-base cells already are; only ``nbins`` int64 per range (and
strand) come back.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from . import _lib
from . import wrappers as _w

# include/bamsignals_abi.h: BSIG_SCALED_MAX_BINS
MAX_BINS = _lib.SCALED_MAX_BINS


def _nbins(nbins):
    if isinstance(nbins, (bool, np.bool_)) or not isinstance(nbins, (int, float, np.integer, np.floating)) \
            or not float(nbins).is_integer():
        raise ValueError("nbins must be a whole number")
    if not 1 <= int(nbins) <= MAX_BINS:
        raise ValueError(f"nbins must lie between 1 and {MAX_BINS}")
    return int(nbins)


def bin_sizes(width, nbins):
    """The cells of every bin, ``(n, nbins)`` int64: bin ``j`` of a range of width ``w`` owns the cells
    ``[ceil(j * w / nbins), ceil((j + 1) * w / nbins))`` -- ``w // nbins`` or one more, none for some bins when
    ``w < nbins``."""
    w = np.asarray(width, dtype=np.int64).reshape(-1, 1)
    edges = -((-np.arange(nbins + 1, dtype=np.int64)[None, :] * w) // nbins)        # ceil(j * w / nbins)
    return np.diff(edges, axis=1)


class ScaledSignals:
    """The scaled-region signal of n ranges, read-only.  ``sums``: ``(n, nbins)`` int64, or ``(n, 2, nbins)`` for
    strand-split 5' ends (sense, antisense): the sums of the cells of every bin.  ``cells``: ``(n, nbins)`` int64, the
    number of cells of every bin (0 for some bins of a range narrower than ``nbins``).  ``width``: the ranges' widths.
    The methods work in exact integer arithmetic; only ``matrix`` returns floats."""

    __slots__ = ("_sums", "_cells", "_width", "_nbins")

    def __init__(self, sums, width, nbins):
        nb = _nbins(nbins)
        s = np.array(sums, dtype=np.int64)
        w = np.array(width, dtype=np.int64).reshape(-1)
        if s.ndim not in (2, 3) or (s.ndim == 3 and s.shape[1] != 2) or s.shape[-1] != nb:
            raise ValueError("sums must have the shape (n, nbins) or (n, 2, nbins)")
        if len(w) != s.shape[0] or (w < 0).any():
            raise ValueError("width must have one entry per range, none of them negative")
        c = bin_sizes(w, nb)
        for a in (s, c, w):
            a.setflags(write=False)
        object.__setattr__(self, "_sums", s)
        object.__setattr__(self, "_cells", c)
        object.__setattr__(self, "_width", w)
        object.__setattr__(self, "_nbins", nb)

    def __setattr__(self, name, value):
        raise AttributeError("ScaledSignals is read-only")

    sums = property(lambda self: self._sums)
    cells = property(lambda self: self._cells)
    width = property(lambda self: self._width)
    nbins = property(lambda self: self._nbins)

    def __len__(self):
        return len(self._width)

    def _den(self):
        """the bins' sizes, shaped as ``sums``"""
        c = self._cells if self._sums.ndim == 2 else self._cells[:, None, :]
        return np.broadcast_to(c, self._sums.shape)

    def mean(self, fractions=False):
        """The mean of every bin's cells, ``sums / cells``, exact: ``(numerator, denominator)`` int64 arrays of
        ``sums``' shape, or with ``fractions=True`` an object array of ``Fraction``s (None for an empty bin)."""
        num, den = self._sums, self._den()
        if not fractions:
            return num, den.copy()
        out = np.empty(num.shape, dtype=object)
        for i in np.ndindex(num.shape):
            out[i] = Fraction(int(num[i]), int(den[i])) if den[i] else None
        return out

    def matrix(self):
        """``sums / cells`` as float64, NaN for an empty bin: the heatmap's matrix, for plotting."""
        den = self._den()
        out = np.full(self._sums.shape, np.nan)
        np.divide(self._sums, den, out=out, where=den > 0)
        return out

    def pooled(self):
        """``(sums.sum(axis=0), cells.sum(axis=0))``: the metaprofile over the ranges, of whatever widths, exact -- bin
        ``j``'s pooled mean is the first over the second (with strands the first has shape ``(2, nbins)``)."""
        return self._sums.sum(axis=0), self._cells.sum(axis=0)

    def __repr__(self):
        return f"ScaledSignals(n={len(self)}, rows={1 if self._sums.ndim == 2 else 2}, nbins={self._nbins})"


def bamScaled(bampath, gr, nbins=100, signal=("coverage", "ends"), ss=False, mapqual=0,  # noqa: N802,N803
              paired_end=None, tlenFilter=None, filteredFlag=-1, verbose=True):
    """The scaled-region signal over the ranges ``gr``: every range cut into ``nbins`` bins (a whole number,
    1 .. ``MAX_BINS``) whatever its width, every bin the sum of its cells.

    ``signal="coverage"``: the cells of ``bamCoverage(bampath, gr, paired_end=...)`` ("ignore" / "extend"); ``ss`` must
    be false.  ``signal="ends"``: the cells of ``bamProfile(bampath, gr, binsize=1, shift=0, ss=ss, paired_end=...)``
    ("ignore" / "filter" / "midpoint"); with ``ss=True`` every range has a sense and an antisense row.  ``paired_end``
    defaults to "ignore".  Returns a ``ScaledSignals`` in the ranges' order."""
    if verbose:
        _w._print_sentence(bampath)
    nb = _nbins(nbins)
    _w._check_gr(gr)
    sig = _w._match_arg(signal, ("coverage", "ends"), "signal")
    choices = ("ignore", "extend") if sig == "coverage" else ("ignore", "filter", "midpoint")
    pe = _w._match_arg(choices if paired_end is None else paired_end, choices, "paired.end")
    if not isinstance(ss, (bool, np.bool_)):
        raise ValueError("ss must be TRUE or FALSE")
    if sig == "coverage" and ss:
        raise ValueError("the scaled regions of coverage have no strands: ss must be FALSE")
    tf = _w.tlenFilter(tlenFilter, pe)
    path = os.path.expanduser(str(bampath))
    if sig == "coverage":
        out = _w.coverage_scaled(path, gr, tf, mapqual, _w.flagMask(pe), filteredFlag, pe == "extend", nb)
    else:
        out = _w.pileup_scaled(path, gr, tf, mapqual, bool(ss), _w.flagMask(pe), filteredFlag, pe == "midpoint", nb)
    if not ss:
        out = out[:, 0, :]
    return ScaledSignals(out, gr.width, nb)
