"""RunSignals: what bamProfile / bamCoverage return with ``runs=True`` -- the per-range signals as runs (value, length),
the counterpart of CountSignals in the form of Bioconductor's RleList (GenomicAlignments::coverage) and of a bedGraph.
The runs are made on the GPU (csrc/runs.hip); the per-base cells never reach the host.

A SEGMENT is one row of one range's signal: ``n_seg = len(sig) * S`` with ``S = 2`` when strand-specific (segment
``2 * i + antisense``), else 1.  Segment k owns runs ``seg_off[k] .. seg_off[k + 1]`` of ``values`` / ``lengths``; its
runs are its maximal stretches of equal consecutive cells, so ``np.repeat(values, lengths)`` over a segment is the row.
Python indices are 0-based; all arrays are read-only."""
from __future__ import annotations

import numpy as np

from .countsignals import CountSignals


class RunSignals:
    def __init__(self, seg_off, values, lengths, ss):
        if not isinstance(ss, (bool, np.bool_)):
            raise ValueError("invalid ss slot")
        self.ss = bool(ss)
        self.seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        self.values = np.ascontiguousarray(values, dtype=np.int32)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        S = 2 if self.ss else 1
        if self.seg_off.ndim != 1 or len(self.seg_off) < 1 or (len(self.seg_off) - 1) % S != 0:
            raise ValueError("seg_off must hold one entry per segment and one more")
        if self.seg_off[0] != 0 or np.any(np.diff(self.seg_off) < 0) or self.seg_off[-1] != len(self.values) \
                or len(self.values) != len(self.lengths):
            raise ValueError("seg_off, values and lengths do not fit each other")
        for a in (self.seg_off, self.values, self.lengths):
            a.setflags(write=False)
        self._S = S

    def __len__(self):
        return (len(self.seg_off) - 1) // self._S

    @property
    def nruns(self):
        """total number of runs"""
        return int(self.seg_off[-1])

    def _segment(self, k):
        a, b = int(self.seg_off[k]), int(self.seg_off[k + 1])
        return self.values[a:b], self.lengths[a:b]

    def _index(self, i):
        n = len(self)
        if not isinstance(i, (int, np.integer)):
            raise TypeError("index a RunSignals with one integer")
        if i < -n or i >= n:
            raise IndexError("range index out of range")
        return int(i) % n if n else 0

    def __getitem__(self, i):
        """(values, lengths) of range i, or ((values, lengths) sense, (values, lengths) antisense) with ss: views"""
        i = self._index(i)
        if self.ss:
            return self._segment(2 * i), self._segment(2 * i + 1)
        return self._segment(i)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def width(self):
        """cells (bases or bins) per range, as CountSignals.width()"""
        ends = np.concatenate([[0], np.cumsum(self.lengths, dtype=np.int64)])[self.seg_off]
        return np.diff(ends)[::self._S].astype(np.int32)

    def decode(self, i):
        """the array CountSignals holds for range i: an int32 vector, or a 2 x n matrix with ss"""
        i = self._index(i)
        if self.ss:
            return np.stack([np.repeat(*self._segment(2 * i)), np.repeat(*self._segment(2 * i + 1))])
        return np.repeat(*self._segment(i))

    def as_countsignals(self):
        return CountSignals([self.decode(i) for i in range(len(self))], self.ss)

    def to_bedgraph(self, path, gr, binsize=1, row=None, zeros=False):
        """Write the runs as a bedGraph: one line ``chrom\\tstart0\\tend\\tvalue`` per run, genomic coordinates 0-based and
        half-open, the ranges in the caller's order.  ``gr`` / ``binsize``: the ranges and bins of the call that made
        the signals; a '-' range is mirrored back to ascending genomic order, the end of a last, short bin is clamped
        to the range's end.  Runs of zeros are skipped unless ``zeros``.  With ss a ``row`` (0 or "sense", 1 or
        "antisense") is required.  Returns the number of lines."""
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
        start, width, strand, chrom = gr.start, gr.width, gr.strand, gr.seqnames
        n_lines = 0
        with open(path, "w") as f:
            for i in range(len(self)):
                v, ln = self._segment(self._S * i + (row or 0))
                w, loc = int(width[i]), int(start[i]) - 1
                if (w + binsize - 1) // binsize != int(ln.sum(dtype=np.int64)):
                    raise ValueError(f"range {i} has {int(ln.sum(dtype=np.int64))} cells: not its width in bins of {binsize}")
                j1 = np.cumsum(ln, dtype=np.int64)
                lo, hi = (j1 - ln) * binsize, np.minimum(j1 * binsize, w)       # bases in range orientation
                if strand[i] == "-":
                    lo, hi, v = (w - hi)[::-1], (w - lo)[::-1], v[::-1]
                keep = slice(None) if zeros else v != 0
                lo, hi, v = lo[keep] + loc, hi[keep] + loc, v[keep]
                f.write("".join(f"{chrom[i]}\t{a}\t{b}\t{x}\n" for a, b, x in zip(lo.tolist(), hi.tolist(), v.tolist())))
                n_lines += len(v)
        return n_lines

    def __repr__(self):
        n = len(self)
        return (f"RunSignals object with {n}{' strand-specific' if self.ss else ''} signal{'s' if n != 1 else ''}, "
                f"{self.nruns} runs")
