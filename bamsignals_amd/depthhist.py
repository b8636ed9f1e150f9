"""bamDepthHist: the depth histogram over ranges -- how the depth is distributed over the targets.

The most common coverage QC questions -- the share of an exome's bases covered at >= 20x, the mean and median depth of a
panel, the depth above which a region is a pile-up artefact, how many positions carry 1, 2, 3 ... 5' ends (the
duplication histogram that library complexity is read from) -- are functions of one small vector: the number of cells
of ``bamCoverage`` / ``bamProfile`` per value.  It is made on the GPU (bsig_coverage_hist / bsig_pileup_hist), where
the per-base cells already are; only its rows come back.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from . import _lib
from . import wrappers as _w

# include/bamsignals_abi.h: BSIG_HIST_MAX_ROWS - 1
MAX_DEPTH = _lib.HIST_MAX_ROWS - 1


class DepthHist:
    """The integers of a depth histogram, read-only.

    ``counts[r]`` (int64, ``maxdepth + 1`` rows): the cells of value r; the last row holds the cells of value
    ``>= maxdepth`` (the overflow row; ``saturated`` says whether it is in use).  ``n``: the number of cells.  ``total``:
    the sum of the cells' TRUE values, also of those in the overflow row.  The methods work in exact integer arithmetic
    and raise ValueError when ``n == 0`` (or ``total == 0`` where they divide by it)."""

    __slots__ = ("_counts", "_n", "_total")

    def __init__(self, counts, n=None, total=None):
        c = np.array(counts, dtype=np.int64).reshape(-1)
        if len(c) < 2:
            raise ValueError("a depth histogram has at least two rows")
        c.setflags(write=False)
        cl = c.tolist()
        n_rows = sum(cl)
        n = n_rows if n is None else int(n)
        if n != n_rows:
            raise ValueError("the rows do not add up to n")
        floor = sum(r * x for r, x in enumerate(cl))          # every cell of the overflow row holds at least maxdepth
        total = floor if total is None else int(total)
        if total < floor or (cl[-1] == 0 and total != floor):
            raise ValueError("total does not fit the rows")
        object.__setattr__(self, "_counts", c)
        object.__setattr__(self, "_n", n)
        object.__setattr__(self, "_total", total)

    def __setattr__(self, name, value):
        raise AttributeError("DepthHist is read-only")

    counts = property(lambda self: self._counts)
    maxdepth = property(lambda self: len(self._counts) - 1)
    n = property(lambda self: self._n)
    total = property(lambda self: self._total)
    saturated = property(lambda self: bool(self._counts[-1] > 0))

    def _need(self):
        if self._n == 0:
            raise ValueError("the histogram is empty (n == 0)")

    def mean(self):
        """``total / n`` as a ``Fraction``: exact even when saturated (``total`` is the sum of the true values)."""
        self._need()
        return Fraction(self._total, self._n)

    def breadth(self, k):
        """The share of cells with value >= k as a ``Fraction`` (0 <= k <= maxdepth): ``breadth(20)`` of a coverage
        histogram is the share of bases covered at 20x or more."""
        self._need()
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 0 or k > self.maxdepth:
            raise ValueError(f"k must be a whole number between 0 and maxdepth ({self.maxdepth})")
        return Fraction(sum(self._counts[int(k):].tolist()), self._n)

    def quantile(self, q):
        """The first value at which the cumulative count reaches ``ceil(q * n)`` (0 <= q <= 1).  A result in the
        overflow row is returned as ``maxdepth`` and means "at least maxdepth"."""
        self._need()
        q = _share(q)
        if q < 0 or q > 1:
            raise ValueError("q must lie between 0 and 1")
        need = -((-q.numerator * self._n) // q.denominator)          # ceil(q * n), exact
        acc = 0
        for r, c in enumerate(self._counts.tolist()):
            acc += c
            if acc >= need:
                return r
        return self.maxdepth

    def median(self):
        return self.quantile(Fraction(1, 2))

    def distinct(self):
        """The cells with a value of 1 or more: for 5' ends, the distinct (position, strand) starts."""
        return sum(self._counts[1:].tolist())

    def duplicate_fraction(self):
        """``1 - distinct / total`` as a ``Fraction``: for 5' ends, the share of reads that repeat another read's
        start."""
        if self._total == 0:
            raise ValueError("the histogram holds no reads (total == 0)")
        return 1 - Fraction(self.distinct(), self._total)

    def __repr__(self):
        return f"DepthHist(maxdepth={self.maxdepth}, n={self._n}, total={self._total}, saturated={self.saturated})"


def _share(x):
    """a share of n as an exact rational; a float is read as the decimal it prints as (0.99 is 99/100)"""
    return Fraction(str(float(x))) if isinstance(x, (float, np.floating)) else Fraction(x)


def _maxdepth(maxdepth):
    if isinstance(maxdepth, (bool, np.bool_)) or not isinstance(maxdepth, (int, float, np.integer, np.floating)) \
            or not float(maxdepth).is_integer():
        raise ValueError("maxdepth must be a whole number")
    v = int(maxdepth)
    if v < 1 or v > MAX_DEPTH:
        raise ValueError(f"maxdepth must be between 1 and {MAX_DEPTH}")
    return v


def bamDepthHist(bampath, gr, maxdepth=1000, signal=("coverage", "ends"), ss=None, paired_end=None,  # noqa: N802,N803
                 tlenFilter=None, mapqual=0, filteredFlag=-1, verbose=True):
    """Histogram of the per-base depth over the ranges ``gr``: ``counts[r]`` is the number of cells of value r, the last
    row (``maxdepth``, at most ``MAX_DEPTH``) the cells of value ``>= maxdepth``.

    ``signal="coverage"``: the cells of ``bamCoverage(bampath, gr, paired_end=...)`` ("ignore" / "extend"); ``ss`` must
    be false.  ``signal="ends"``: the cells of ``bamProfile(bampath, gr, binsize=1, shift=0, ss=ss, paired_end=...)``
    ("ignore" / "filter" / "midpoint"); ``ss`` (default True) makes every (base, strand) a cell of its own, which is what
    a duplication histogram counts; with ``ss=False`` a cell is a base and its value the sum of both strands.
    ``paired_end`` defaults to "ignore".  A repeated range counts twice, the bases of an overhang are cells of value 0,
    the ranges' strands do not matter.  Returns a ``DepthHist``."""
    if verbose:
        _w._print_sentence(bampath)
    v = _maxdepth(maxdepth)
    _w._check_gr(gr)
    sig = _w._match_arg(signal, ("coverage", "ends"), "signal")
    choices = ("ignore", "extend") if sig == "coverage" else ("ignore", "filter", "midpoint")
    pe = _w._match_arg(choices if paired_end is None else paired_end, choices, "paired.end")
    if ss is None:
        ss = sig == "ends"
    if not isinstance(ss, (bool, np.bool_)):
        raise ValueError("ss must be TRUE or FALSE")
    if sig == "coverage" and ss:
        raise ValueError("the depth histogram of coverage has no strands: ss must be FALSE")
    tf = _w.tlenFilter(tlenFilter, pe)
    path = os.path.expanduser(str(bampath))
    if sig == "coverage":
        out = _w.coverage_hist(path, gr, tf, mapqual, _w.flagMask(pe), filteredFlag, pe == "extend", v)
    else:
        out = _w.pileup_hist(path, gr, tf, mapqual, bool(ss), _w.flagMask(pe), filteredFlag, pe == "midpoint", v)
    return DepthHist(out[:v + 1], n=int(out[v + 1]), total=int(out[v + 2]))
