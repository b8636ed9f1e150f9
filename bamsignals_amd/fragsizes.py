"""bamFragSizes: the fragment-length histogram over ranges -- the data's own value for ``tlenFilter``.

Every paired-end call takes a ``tlenFilter`` whose default, (0, 1000), is a guess (R/wrappers.R:84-98).  Paired-end data
carries the fragment length in every record: the histogram of |tlen| over the first reads of the proper pairs whose
position lies in the ranges is the nucleosome ladder of ATAC-seq / MNase, the insert size over peaks, and the interval
that holds 99 % of it is the filter.  The histogram is made on the GPU (bsig_pileup_frag); only its rows come back.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np

from . import _lib
from . import wrappers as _w

# include/bamsignals_abi.h: BSIG_FRAG_MAX_ROWS
MAX_ROWS = _lib.FRAG_MAX_ROWS


class FragSizes:
    """The integers of a fragment-length histogram, read-only.

    ``counts[r]`` (int64): the fragments with ``|tlen| // lenbin == r``.  ``lengths[r] = r * lenbin``: the first length
    of row r.  ``n``: the total.  The methods work in exact integer arithmetic on ``counts`` and raise ValueError when
    ``n == 0``."""

    __slots__ = ("_counts", "_lenbin", "_lengths", "_n")

    def __init__(self, counts, lenbin=1):
        c = np.array(counts, dtype=np.int64).reshape(-1)
        c.setflags(write=False)
        lb = _lenbin(lenbin)
        lengths = np.arange(len(c), dtype=np.int64) * lb
        lengths.setflags(write=False)
        object.__setattr__(self, "_counts", c)
        object.__setattr__(self, "_lenbin", lb)
        object.__setattr__(self, "_lengths", lengths)
        object.__setattr__(self, "_n", sum(int(x) for x in c))

    def __setattr__(self, name, value):
        raise AttributeError("FragSizes is read-only")

    counts = property(lambda self: self._counts)
    lenbin = property(lambda self: self._lenbin)
    lengths = property(lambda self: self._lengths)
    n = property(lambda self: self._n)

    def _need(self):
        if self._n == 0:
            raise ValueError("the histogram is empty (n == 0)")

    def mode(self):
        """The first length of the fullest row, the first one on ties."""
        self._need()
        return int(np.argmax(self._counts)) * self._lenbin

    def quantile(self, q):
        """The first length of the first row at which the cumulative count reaches ``ceil(q * n)`` (0 <= q <= 1)."""
        self._need()
        q = _share(q)
        if q < 0 or q > 1:
            raise ValueError("q must lie between 0 and 1")
        need = -((-q.numerator * self._n) // q.denominator)          # ceil(q * n), exact
        acc = 0
        for r, c in enumerate(self._counts.tolist()):
            acc += c
            if acc >= need:
                return r * self._lenbin
        return (len(self._counts) - 1) * self._lenbin

    def median(self):
        return self.quantile(Fraction(1, 2))

    def mean(self):
        """``sum(length * count) / n`` as a ``Fraction``.  A row stands for its FIRST length: with ``lenbin > 1`` the
        mean is that of the rows' first lengths, up to ``lenbin - 1`` below the fragments' own."""
        self._need()
        return Fraction(sum(r * self._lenbin * c for r, c in enumerate(self._counts.tolist())), self._n)

    def tlen_filter(self, mass=0.99):
        """``(lo, hi)``: the shortest central interval that leaves at most ``(1 - mass) / 2`` of ``n`` outside on each
        side -- rows are dropped from either end while the fragments dropped on that side stay within that share.
        ``lo`` is a row's first length and ``hi`` a row's last, so the pair is ready to pass as ``tlenFilter``."""
        self._need()
        m = _share(mass)
        if m <= 0 or m > 1:
            raise ValueError("mass must lie in (0, 1]")
        tail = (1 - m) / 2
        allowed = (tail.numerator * self._n) // tail.denominator     # floor(tail * n) fragments a side, exact
        c = self._counts.tolist()
        lo, out = 0, 0
        while lo < len(c) - 1 and out + c[lo] <= allowed:
            out += c[lo]
            lo += 1
        hi, out = len(c) - 1, 0
        while hi > lo and out + c[hi] <= allowed:
            out += c[hi]
            hi -= 1
        return lo * self._lenbin, (hi + 1) * self._lenbin - 1

    def __repr__(self):
        return f"FragSizes(rows={len(self._counts)}, lenbin={self._lenbin}, n={self._n})"


def _share(x):
    """a share of n as an exact rational; a float is read as the decimal it prints as (0.99 is 99/100)"""
    return Fraction(str(float(x))) if isinstance(x, (float, np.floating)) else Fraction(x)


def _lenbin(lenbin):
    if isinstance(lenbin, (bool, np.bool_)) or not isinstance(lenbin, (int, float, np.integer, np.floating)) \
            or not float(lenbin).is_integer():
        raise ValueError("lenbin must be a whole number of bases")
    b = int(lenbin)
    if b < 1:
        raise ValueError("lenbin must be greater or equal to 1")
    return b


def bamFragSizes(bampath, gr, tlenFilter=None, lenbin=1, paired_end=("filter", "midpoint"), mapqual=0,  # noqa: N802,N803
                 filteredFlag=-1, verbose=True):
    """Histogram of the fragment lengths |tlen| over the ranges ``gr``: row r counts the lengths ``r * lenbin ..
    (r + 1) * lenbin - 1`` inside ``tlenFilter`` (None: (0, 1000)), ``tlenFilter[1] // lenbin + 1`` rows (at most
    ``MAX_ROWS``).

    ``counts[r]`` is the sum over the ranges of ``bamCount(bampath, gr[i], paired_end=paired_end, tlenFilter=row r's
    lengths)``: a fragment counts through the first read of its proper pair, where ``bamCount`` puts it -- at its 5' end
    ("filter") or at its midpoint ("midpoint") -- once per range that holds that position; the ranges' strands do not
    matter.  ``mapqual`` and ``filteredFlag`` filter the reads as in ``bamCount``.  Returns a ``FragSizes``; the data's
    own filter for the counting calls is ``bamFragSizes(...).tlen_filter(0.99)``."""
    if verbose:
        _w._print_sentence(bampath)
    b = _lenbin(lenbin)
    _w._check_gr(gr)
    pe = _w._match_arg(paired_end, ("filter", "midpoint"), "paired.end")
    tf = _w.tlenFilter(tlenFilter, pe)
    if tf[1] // b + 1 > MAX_ROWS:
        raise ValueError(f"tlenFilter[1] // lenbin + 1 = {tf[1] // b + 1} rows, at most {MAX_ROWS} fit: choose a wider lenbin")
    out = _w.pileup_frag(os.path.expanduser(str(bampath)), gr, tf, mapqual, _w.flagMask(pe), filteredFlag,
                         pe == "midpoint", b)
    return FragSizes(out, b)
