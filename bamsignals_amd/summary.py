"""bamSummary: every range's own depth summary -- sum, max, summit and breadth at thresholds.

What a set of peaks or capture targets is usually asked: the height and the summit position of every peak and the reads
in it; the mean depth of every target and its bases at >= 1x / 10x / 20x / 30x.  All of it is a few integers per range
of the cells of ``bamCoverage`` / ``bamProfile``.  They are made on the GPU (bsig_coverage_summary /
bsig_pileup_summary), where the per-base cells already are; only ``3 + K`` int64 per range (and strand) come back.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from . import _lib
from . import wrappers as _w

# include/bamsignals_abi.h: BSIG_SUMMARY_MAX_THRESHOLDS
MAX_THRESHOLDS = _lib.SUMMARY_MAX_THRESHOLDS


def _thresholds(thresholds):
    try:
        ts = list(thresholds)
    except TypeError:
        raise ValueError("thresholds must be a sequence of whole numbers") from None
    out = []
    for t in ts:
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)) \
                or not float(t).is_integer():
            raise ValueError("thresholds must be whole numbers")
        out.append(int(t))
    if len(out) > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds")
    if any(t < 1 or t > 2**31 - 1 for t in out):
        raise ValueError("thresholds must lie between 1 and 2^31 - 1")
    if any(b <= a for a, b in zip(out[:-1], out[1:])):
        raise ValueError("thresholds must be strictly increasing")
    return tuple(out)


class RangeSummary:
    """The integers of per-range summaries, read-only.  With n ranges, K thresholds and, for strand-split 5' ends, the
    two rows sense / antisense (shape ``(n, 2)``, otherwise ``(n,)``):

    ``sum``, ``max``: of the range's cells.  ``summit``: the 0-based index of the first cell holding the max, in range
    orientation (an index into ``bamCoverage(...)[i]`` / ``bamProfile(...)[i][row]``); 0 for an all-zero range, -1 for
    a range without width.  ``covered``: shape ``(n[, 2], K)``, the cells ``>= thresholds[k]``.  ``width``: the ranges'
    widths.  All int64; the methods work in exact integer arithmetic."""

    __slots__ = ("_sum", "_max", "_summit", "_covered", "_width", "_thresholds", "_start", "_neg")

    def __init__(self, sum, max, summit, covered, width, thresholds, start=None, strand=None):  # noqa: A002
        def ro(a):
            a = np.array(a, dtype=np.int64)
            a.setflags(write=False)
            return a
        s, m, p, c, w = ro(sum), ro(max), ro(summit), ro(covered), ro(width).reshape(-1)
        th = _thresholds(thresholds)
        if s.ndim not in (1, 2) or (s.ndim == 2 and s.shape[1] != 2) or m.shape != s.shape or p.shape != s.shape:
            raise ValueError("sum, max and summit must share the shape (n,) or (n, 2)")
        if c.shape != s.shape + (len(th),):
            raise ValueError("covered must have the shape of sum with one more axis of len(thresholds)")
        if len(w) != s.shape[0]:
            raise ValueError("width must have one entry per range")
        object.__setattr__(self, "_sum", s)
        object.__setattr__(self, "_max", m)
        object.__setattr__(self, "_summit", p)
        object.__setattr__(self, "_covered", c)
        object.__setattr__(self, "_width", w)
        object.__setattr__(self, "_thresholds", th)
        object.__setattr__(self, "_start", None if start is None else ro(start).reshape(-1))
        neg = None if strand is None else np.array([x in ("-", -1) for x in strand], dtype=bool)
        object.__setattr__(self, "_neg", neg)
        if (self._start is None) != (neg is None) or (neg is not None and (len(neg) != len(w) or len(self._start) != len(w))):
            raise ValueError("start and strand come together, one entry per range")

    def __setattr__(self, name, value):
        raise AttributeError("RangeSummary is read-only")

    sum = property(lambda self: self._sum)
    max = property(lambda self: self._max)
    summit = property(lambda self: self._summit)
    covered = property(lambda self: self._covered)
    width = property(lambda self: self._width)
    thresholds = property(lambda self: self._thresholds)

    def __len__(self):
        return len(self._width)

    def _w(self):
        """the widths, shaped to divide ``sum``"""
        return self._width if self._sum.ndim == 1 else self._width[:, None]

    def mean(self, fractions=False):
        """The mean depth ``sum / width`` per range, exact: ``(numerator, denominator)`` int64 arrays of ``sum``'s shape,
        or with ``fractions=True`` an object array of ``Fraction``s (None for a range without width)."""
        num, den = self._sum, np.broadcast_to(self._w(), self._sum.shape)
        return _fractions(num, den) if fractions else (num, den.copy())

    def _k(self, t):
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) or int(t) not in self._thresholds:
            raise ValueError(f"{t!r} is not one of the thresholds asked for {self._thresholds}")
        return self._thresholds.index(int(t))

    def breadth(self, t, fractions=False):
        """The share of the range's cells with value >= t, exact, as ``mean`` returns it.  ``t`` must be one of
        ``thresholds``: ValueError otherwise."""
        num = self._covered[..., self._k(t)]
        den = np.broadcast_to(self._w(), num.shape)
        return _fractions(num, den) if fractions else (num, den.copy())

    def summit_position(self):
        """The summits as 1-based genomic coordinates, ``GRanges``' convention: ``start + summit`` on a '+' or '*'
        range, ``end - summit`` on a '-' range (whose cells are mirrored); 0 where there is no summit (no width)."""
        if self._start is None:
            raise ValueError("this summary does not know its ranges (made without start and strand)")
        start, neg, w = self._start, self._neg, self._width
        if self._summit.ndim == 2:
            start, neg, w = start[:, None], neg[:, None], w[:, None]
        pos = np.where(neg, start + w - 1 - self._summit, start + self._summit)
        return np.where(self._summit < 0, 0, pos)

    def failing(self, t, min_breadth):
        """The indices of the ranges whose breadth at ``t`` is below ``min_breadth`` (a share between 0 and 1; a float is
        read as the decimal it prints as), compared exactly; with strands, on either strand.  A range without width
        fails."""
        q = Fraction(str(float(min_breadth))) if isinstance(min_breadth, (float, np.floating)) else Fraction(min_breadth)
        if q < 0 or q > 1:
            raise ValueError("min_breadth must lie between 0 and 1")
        num, den = self.breadth(t)
        # num / den < q  <=>  num * q.denominator < q.numerator * den  (object arithmetic: no 64-bit wrap)
        bad = (num.astype(object) * q.denominator < den.astype(object) * q.numerator) | (den == 0)
        if bad.ndim == 2:
            bad = bad.any(axis=1)
        return np.flatnonzero(bad.astype(bool))

    def __repr__(self):
        return f"RangeSummary(n={len(self)}, rows={1 if self._sum.ndim == 1 else 2}, thresholds={self._thresholds})"


def _fractions(num, den):
    out = np.empty(num.shape, dtype=object)
    for i in np.ndindex(num.shape):
        out[i] = Fraction(int(num[i]), int(den[i])) if den[i] else None
    return out


def bamSummary(bampath, gr, thresholds=(1, 10, 20, 30), signal=("coverage", "ends"), ss=False, mapqual=0,  # noqa: N802,N803
               paired_end=None, tlenFilter=None, filteredFlag=-1, verbose=True):
    """Per-range summaries of the per-base depth over the ranges ``gr``: for every range the sum, the max, the summit
    and the number of cells at or above each of ``thresholds`` (whole numbers >= 1, strictly increasing, at most
    ``MAX_THRESHOLDS``; may be empty).

    ``signal="coverage"``: the cells of ``bamCoverage(bampath, gr, paired_end=...)`` ("ignore" / "extend"); ``ss`` must
    be false.  ``signal="ends"``: the cells of ``bamProfile(bampath, gr, binsize=1, shift=0, ss=ss, paired_end=...)``
    ("ignore" / "filter" / "midpoint"); with ``ss=True`` every range has a sense and an antisense row.  ``paired_end``
    defaults to "ignore".  Returns a ``RangeSummary`` in the ranges' order."""
    if verbose:
        _w._print_sentence(bampath)
    th = _thresholds(thresholds)
    _w._check_gr(gr)
    sig = _w._match_arg(signal, ("coverage", "ends"), "signal")
    choices = ("ignore", "extend") if sig == "coverage" else ("ignore", "filter", "midpoint")
    pe = _w._match_arg(choices if paired_end is None else paired_end, choices, "paired.end")
    if not isinstance(ss, (bool, np.bool_)):
        raise ValueError("ss must be TRUE or FALSE")
    if sig == "coverage" and ss:
        raise ValueError("the range summary of coverage has no strands: ss must be FALSE")
    tf = _w.tlenFilter(tlenFilter, pe)
    path = os.path.expanduser(str(bampath))
    if sig == "coverage":
        out = _w.coverage_summary(path, gr, tf, mapqual, _w.flagMask(pe), filteredFlag, pe == "extend", th)
    else:
        out = _w.pileup_summary(path, gr, tf, mapqual, bool(ss), _w.flagMask(pe), filteredFlag, pe == "midpoint", th)
    if not ss:
        out = out[:, 0, :]
    return RangeSummary(out[..., 0], out[..., 1], out[..., 2], out[..., _lib.SUMMARY_FIXED:], gr.width, th,
                        start=gr.start, strand=gr.strand)
