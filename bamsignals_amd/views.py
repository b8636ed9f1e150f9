"""bamViews: where is the signal?  The stretches of every range whose coverage (or 5'-end pileup) lies at or above a depth,
each with its sum, its max and its summit -- callable regions (mosdepth --quantize, GATK CallableLoci), the candidate
peaks of a pileup, IRanges' ``slice(coverage, lower)`` with viewSums / viewMaxs / viewWhichMaxs.  Found on the GPU
(csrc/views.hip); the per-base cells never reach the host, only 24 bytes per view do.

A cell (a base, or a bin with ``binsize``) is IN iff ``lower <= v <= upper``; a VIEW is a maximal stretch of consecutive
in-cells of one SEGMENT, one row of one range's signal: ``n_seg = len(sig) * S`` with ``S = 2`` when strand-specific
(segment ``2 * i + antisense``), else 1.  Segment k owns views ``seg_off[k] .. seg_off[k + 1]``; ``start`` and ``summit``
are 0-based cell indices inside the segment in range orientation (a '-' range is mirrored, as in bamProfile), ``summit``
the FIRST cell that holds ``max`` (bamSummary's tie rule).  All arrays are read-only."""
from __future__ import annotations

import os
import warnings

import numpy as np

from . import wrappers as _w
from .granges import GRanges

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def _threshold(value, name):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not float(value).is_integer():
        raise ValueError(f"{name} must be a whole number")
    v = int(value)
    if v < INT32_MIN or v > INT32_MAX:
        raise ValueError(f"{name} must lie in the int32 range")
    return v


def _thresholds(lower, upper):
    lo = _threshold(lower, "lower")
    hi = INT32_MAX if upper is None else _threshold(upper, "upper")
    if lo > hi:
        raise ValueError("lower must not be above upper")
    return lo, hi


class SignalViews:
    FIELDS = ("start", "width", "sum", "max", "summit")

    def __init__(self, seg_off, start, width, sum, max, summit, ss):  # noqa: A002
        if not isinstance(ss, (bool, np.bool_)):
            raise ValueError("invalid ss slot")
        self.ss = bool(ss)
        self.seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        self.start = np.ascontiguousarray(start, dtype=np.int32)
        self.width = np.ascontiguousarray(width, dtype=np.int32)
        self.sum = np.ascontiguousarray(sum, dtype=np.int64)
        self.max = np.ascontiguousarray(max, dtype=np.int32)
        self.summit = np.ascontiguousarray(summit, dtype=np.int32)
        S = 2 if self.ss else 1
        if self.seg_off.ndim != 1 or len(self.seg_off) < 1 or (len(self.seg_off) - 1) % S != 0:
            raise ValueError("seg_off must hold one entry per segment and one more")
        n = len(self.start)
        if self.seg_off[0] != 0 or np.any(np.diff(self.seg_off) < 0) or self.seg_off[-1] != n \
                or any(a.ndim != 1 or len(a) != n for a in (self.width, self.sum, self.max, self.summit)):
            raise ValueError("seg_off and the view arrays do not fit each other")
        if n:
            end = self.start.astype(np.int64) + self.width
            if np.any(self.start < 0) or np.any(self.width < 1) or np.any(self.summit < self.start) or np.any(self.summit >= end):
                raise ValueError("a view needs a start >= 0, a width >= 1 and its summit inside it")
            apart = self.start[1:] > end[:-1]                       # ascending with a cell between: inside a segment
            apart[self.seg_off[1:-1][(self.seg_off[1:-1] > 0) & (self.seg_off[1:-1] < n)] - 1] = True
            if not np.all(apart):
                raise ValueError("the views of a segment must ascend and not touch")
        for a in (self.seg_off, self.start, self.width, self.sum, self.max, self.summit):
            a.setflags(write=False)
        self._S = S

    def __len__(self):
        return (len(self.seg_off) - 1) // self._S

    @property
    def nviews(self):
        """total number of views"""
        return int(self.seg_off[-1])

    def _segment(self, k):
        a, b = int(self.seg_off[k]), int(self.seg_off[k + 1])
        return {f: getattr(self, f)[a:b] for f in self.FIELDS}

    def _index(self, i):
        n = len(self)
        if not isinstance(i, (int, np.integer)):
            raise TypeError("index a SignalViews with one integer")
        if i < -n or i >= n:
            raise IndexError("range index out of range")
        return int(i) % n if n else 0

    def __getitem__(self, i):
        """the views of range i: a dict of array views (start, width, sum, max, summit), or (sense, antisense) with ss"""
        i = self._index(i)
        if self.ss:
            return self._segment(2 * i), self._segment(2 * i + 1)
        return self._segment(i)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def counts(self):
        """views per range: an int64 vector, or a 2 x n matrix (rows sense, antisense) with ss"""
        c = np.diff(self.seg_off)
        return c.reshape(-1, 2).T.copy() if self.ss else c

    def _segment_of_view(self):
        return np.repeat(np.arange(len(self.seg_off) - 1), np.diff(self.seg_off))

    def wider_than(self, minwidth):
        """A new SignalViews without the views narrower than ``minwidth`` cells."""
        keep = self.width >= int(minwidth)
        seg_off = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])[self.seg_off]
        return SignalViews(seg_off, *(getattr(self, f)[keep] for f in self.FIELDS), self.ss)

    def merged(self, maxgap):
        """A new SignalViews in which the views of one segment that are separated by at most ``maxgap`` cells are joined:
        ``start`` is the first part's, ``width`` spans the parts and the gaps between them, ``max`` is the largest part
        max and ``summit`` the first summit holding it.  ``sum`` is the sum of the PARTS: the cells of a gap lie outside
        ``[lower, upper]`` and are not added (so ``sum / width`` is not the mean depth of a joined view)."""
        maxgap = int(maxgap)
        if maxgap < 0:
            raise ValueError("maxgap must not be negative")
        n = self.nviews
        if n == 0:
            return SignalViews(self.seg_off, *(getattr(self, f) for f in self.FIELDS), self.ss)
        end = self.start.astype(np.int64) + self.width
        head = np.ones(n, bool)                                     # the first part of a joined view
        head[1:] = (self.start[1:] - end[:-1] > maxgap) | (np.diff(self._segment_of_view()) != 0)
        at = np.flatnonzero(head)
        seg_off = np.concatenate([[0], np.cumsum(head, dtype=np.int64)])[self.seg_off]
        last = np.concatenate([at[1:], [n]]) - 1
        gmax = np.maximum.reduceat(self.max, at)
        group = np.cumsum(head) - 1
        holder = np.where(self.max == gmax[group], np.arange(n), n)   # parts that hold the joined max: the first one
        first = np.minimum.reduceat(holder, at)
        return SignalViews(seg_off, self.start[at], (end[last] - self.start[at]).astype(np.int32), np.add.reduceat(self.sum, at), gmax,
                           self.summit[first], self.ss)

    def _rows(self, gr, binsize, row):
        binsize = int(binsize)
        if binsize < 1:
            raise ValueError("provide a binsize greater or equal to 1")
        if len(gr) != len(self):
            raise ValueError("gr must be the ranges the signals were made for")
        if self.ss:
            if row is None:
                raise ValueError("strand-specific signals: choose a row (0 sense, 1 antisense)")
            row = {"sense": 0, "antisense": 1}.get(row, row)
            if row not in (0, 1):
                raise ValueError("row must be 0 (sense) or 1 (antisense)")
        elif row not in (None, 0):
            raise ValueError("signals without strands have one row")
        return binsize, row or 0

    def _genomic(self, gr, binsize, row):
        """per view of the chosen row, ranges in the caller's order and ascending inside a range: (range index, view index
        inside its segment, 0-based genomic start, end (half-open), 0-based genomic first base of the summit cell, view)"""
        binsize, row = self._rows(gr, binsize, row)
        segs = np.arange(len(self)) * self._S + row
        a, b = self.seg_off[segs], self.seg_off[segs + 1]
        rng = np.repeat(np.arange(len(self)), b - a)
        view = np.concatenate([np.arange(x, y) for x, y in zip(a, b)]).astype(np.int64) if len(rng) else np.zeros(0, np.int64)
        j = view - a[rng]
        w = np.asarray(gr.width, np.int64)[rng]
        loc = np.asarray(gr.start, np.int64)[rng] - 1
        start, width, summit = self.start[view].astype(np.int64), self.width[view].astype(np.int64), self.summit[view].astype(np.int64)
        if np.any((start + width - 1) * binsize >= w):
            raise ValueError(f"a view lies beyond its range's width in bins of {binsize}")
        lo, hi = start * binsize, np.minimum((start + width) * binsize, w)        # bases in range orientation
        s_lo, s_hi = summit * binsize, np.minimum((summit + 1) * binsize, w)
        minus = np.asarray([s == "-" for s in gr.strand], bool)[rng] if len(rng) else np.zeros(0, bool)
        g_lo, g_hi = np.where(minus, w - hi, lo) + loc, np.where(minus, w - lo, hi) + loc
        g_summit = np.where(minus, w - s_hi, s_lo) + loc
        # a '-' range mirrored back: its views in ascending genomic order
        order = np.lexsort((np.where(minus, -j, j), rng))
        return tuple(x[order] for x in (rng, j, g_lo, g_hi, g_summit, view))

    def to_granges(self, gr, binsize=1, row=None):
        """The views as genomic ranges: ``(GRanges, columns)``.  ``gr`` / ``binsize``: the ranges and bins of the call
        that made the views.  The GRanges holds one 1-based range per view with its range's strand, the ranges in the
        caller's order and ascending inside each (a '-' range is mirrored back; the end of a last, short bin is clamped
        to the range's end); ``columns`` is a dict of arrays in the same order: ``range`` (index into ``gr``), ``view``
        (index of the view inside its segment), ``sum``, ``max`` and ``summit`` (1-based genomic position of the first
        base of the summit cell).  With ss a ``row`` (0 or "sense", 1 or "antisense") is required."""
        rng, j, g_lo, g_hi, g_summit, view = self._genomic(gr, binsize, row)
        out = GRanges([gr.seqnames[i] for i in rng], g_lo + 1, width=g_hi - g_lo, strand=[gr.strand[i] for i in rng])
        return out, dict(range=rng, view=j, sum=self.sum[view], max=self.max[view], summit=g_summit + 1)

    def to_bed(self, path, gr, binsize=1, row=None):
        """Write the views as BED6+2: ``chrom  chromStart  chromEnd  range{i}_{j}  max  strand  sum  summit`` -- 0-based
        half-open coordinates as ``to_granges`` gives them, ``i`` the range, ``j`` the view inside its segment, the score
        the view's max, ``summit`` the offset of the summit cell's first base from chromStart (narrowPeak's peak column).
        Returns the number of lines."""
        rng, j, g_lo, g_hi, g_summit, view = self._genomic(gr, binsize, row)
        chrom, strand = gr.seqnames, gr.strand
        with open(path, "w") as f:
            f.write("".join(f"{chrom[i]}\t{a}\t{b}\trange{i}_{k}\t{m}\t{strand[i]}\t{s}\t{t - a}\n"
                            for i, k, a, b, t, m, s in zip(rng.tolist(), j.tolist(), g_lo.tolist(), g_hi.tolist(), g_summit.tolist(),
                                                           self.max[view].tolist(), self.sum[view].tolist())))
        return len(rng)

    def __repr__(self):
        n = len(self)
        return (f"SignalViews object with {n}{' strand-specific' if self.ss else ''} signal{'s' if n != 1 else ''}, "
                f"{self.nviews} views")


def bamViews(bampath, gr, lower, upper=None, signal=("coverage", "ends"), mapqual=0, binsize=1, ss=False, shift=0,  # noqa: N802
             paired_end="ignore", tlenFilter=None, filteredFlag=-1, fragLength=None, verbose=True, *, splice=False):  # noqa: N803
    """For each range, the stretches whose signal lies in ``[lower, upper]``, with their sum, max and summit: a SignalViews.

    ``lower`` / ``upper``: whole numbers in the int32 range, ``lower <= upper``; ``upper=None`` means 2^31 - 1, "at or
    above ``lower``".  ``signal="coverage"``: the cells of ``bamCoverage(bampath, gr, ...)`` with the same ``mapqual``,
    ``binsize``, ``ss``, ``paired_end`` ("ignore" or "extend"), ``tlenFilter``, ``filteredFlag`` and ``fragLength``;
    ``shift`` must be 0.  ``signal="ends"``: the cells of ``bamProfile`` -- the 5' ends -- with ``binsize``, ``ss``,
    ``shift`` and ``paired_end`` ("ignore", "filter" or "midpoint"); it takes no ``fragLength``.  With ``binsize`` a cell
    is a bin and the thresholds are compared with the bin's sum.  ``splice=True`` (``signal="coverage"`` only): the cells of
    ``bamCoverage(..., splice=True)``, the coverage that skips the reads' ``N`` gaps.  The views are found on the GPU; only
    they are downloaded."""
    lo, hi = _thresholds(lower, upper)
    sig = _w._match_arg(signal, ("coverage", "ends"), "signal")
    if isinstance(shift, (bool, np.bool_)) or not isinstance(shift, (int, np.integer)):
        raise ValueError("shift must be a whole number of bases")
    if sig == "coverage":
        if shift != 0:
            raise ValueError('signal="coverage" has no shift: a read covers the bases it covers')
        sp = _w._splice(splice, paired_end, ("ignore", "extend"), fragLength)
        frag = _w._frag_length(fragLength)
        pe = _w._match_arg(paired_end, ("ignore", "extend"), "paired.end")
        if frag and pe != "ignore":
            raise ValueError('fragLength resizes single-end reads: with paired_end="extend" a fragment already has its length')
        b = _w._coverage_binsize(binsize)
    else:
        if not isinstance(splice, (bool, np.bool_)):
            raise ValueError("splice must be True or False")
        if splice:
            raise ValueError('splice with signal="ends": a block\'s start is not a read\'s 5\' end')
        if fragLength is not None:
            raise ValueError('signal="ends" takes no fragLength: a 5\' end is one base')
        pe = _w._match_arg(paired_end, ("ignore", "filter", "midpoint"), "paired.end")
        b = int(binsize)
        if b < 1:
            raise ValueError("provide a binsize greater or equal to 1")
    _w._check_gr(gr)
    if verbose:
        _w._print_sentence(bampath)
    if b > 1 and np.any(gr.width % b != 0):
        warnings.warn("some ranges' widths are not a multiple of the selected\n"
                      "             binsize, some bins will correspond to less than binsize basepairs")
    path, tf = os.path.expanduser(str(bampath)), _w.tlenFilter(tlenFilter, pe)
    if sig == "coverage":
        return _w.coverage_views(path, gr, tf, lo, hi, mapqual, _w.flagMask(pe), filteredFlag, pe == "extend", binsize=b, ss=bool(ss),
                                 frag_len=frag, **(dict(spliced=True) if sp else {}))
    return _w.pileup_views(path, gr, tf, lo, hi, mapqual, b, int(shift), bool(ss), _w.flagMask(pe), filteredFlag, pe == "midpoint")
