"""bamJunctions: which introns do the reads support, and how well?  Every ``N`` gap of a read is a splice junction; for each
range this gives the distinct junctions that lie within it, the number of reads across each -- split by strand with ``ss`` --
and the largest anchor among them: ``GenomicAlignments::summarizeJunctions`` (score, plus_score, minus_score), STAR's
``SJ.out.tab`` (read count, maximum overhang), ``regtools junctions extract -a`` (the anchor filter).  Counted on the GPU
(csrc/junctions.hip) from the junction table that the file's spliced reads keep -- the same resident set
``bamCoverage(splice=True)`` uses --; no CIGAR is walked on the host and only the distinct junctions, 20 bytes each, come back.

A gap is what ``bamCoverage(splice=True)`` skips: a maximal stretch of ``N`` operations (neighbouring ``N`` and ``N``
separated only by ``I S H P`` merge; an unmapped read has none).  A read's ANCHOR at a junction is the smaller of the
aligned reference bases right before the gap and right behind it (up to the read's previous / next gap or its first / last
base; ``D`` counts, ``I`` does not; 0 where the gap opens or closes the read).  The junction's strand from the ``XS`` / ``ts``
tags, the paired-end rules (``tlenFilter``, mate-aware strand) and junctions that merely overlap a range are not built.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from . import wrappers as _w
from .granges import GRanges


class Junctions:
    """The junctions of n ranges, read-only.  Range i owns entries ``seg_off[i] .. seg_off[i + 1]`` of ``start``, ``end``
    (1-based, inclusive: the intron's first and last base, GRanges' convention), ``count`` (int64; shape ``(n,)``, or
    ``(n, 2)`` with ss: reads whose strand agrees with the range's, ``*`` counted as ``+``, and reads on the other one) and
    ``max_anchor``; inside a range they ascend by start, then end."""

    FIELDS = ("start", "end", "count", "max_anchor")

    def __init__(self, seg_off, start, end, count, max_anchor, ss):
        if not isinstance(ss, (bool, np.bool_)):
            raise ValueError("invalid ss slot")
        self.ss = bool(ss)
        self.seg_off = np.array(seg_off, dtype=np.int64)
        self.start = np.array(start, dtype=np.int64)
        self.end = np.array(end, dtype=np.int64)
        self.count = np.array(count, dtype=np.int64)
        self.max_anchor = np.array(max_anchor, dtype=np.int64)
        n = len(self.start)
        if self.seg_off.ndim != 1 or len(self.seg_off) < 1 or self.seg_off[0] != 0 or np.any(np.diff(self.seg_off) < 0) \
                or self.seg_off[-1] != n:
            raise ValueError("seg_off must hold one entry per range and one more, from 0 to the number of junctions")
        if self.count.shape != ((n, 2) if self.ss else (n,)) or any(a.shape != (n,) for a in (self.start, self.end, self.max_anchor)):
            raise ValueError("the junction arrays do not fit each other")
        if n and (np.any(self.end < self.start) or np.any(self.count < 0) or np.any(self.max_anchor < 0)):
            raise ValueError("a junction needs start <= end, counts and an anchor that are not negative")
        for a in (self.seg_off, self.start, self.end, self.count, self.max_anchor):
            a.setflags(write=False)

    def __len__(self):
        return len(self.seg_off) - 1

    @property
    def njunctions(self):
        """total number of junctions"""
        return int(self.seg_off[-1])

    def support(self):
        """reads per junction, strands summed (int64)"""
        return self.count.sum(axis=1) if self.ss else self.count

    def __getitem__(self, i):
        """the junctions of range i: a dict of array views (start, end, count, max_anchor)"""
        n = len(self)
        if not isinstance(i, (int, np.integer)):
            raise TypeError("index a Junctions with one integer")
        if i < -n or i >= n:
            raise IndexError("range index out of range")
        i = int(i) % n
        a, b = int(self.seg_off[i]), int(self.seg_off[i + 1])
        return {f: getattr(self, f)[a:b] for f in self.FIELDS}

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def with_support(self, k):
        """A new Junctions with the junctions that at least ``k`` reads support (strands summed)."""
        keep = self.support() >= int(k)
        seg_off = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])[self.seg_off]
        return Junctions(seg_off, *(getattr(self, f)[keep] for f in self.FIELDS), self.ss)

    def _range_of(self, gr):
        _w._check_gr(gr)
        if len(gr) != len(self):
            raise ValueError("gr must be the ranges the junctions were counted for")
        return np.repeat(np.arange(len(self)), np.diff(self.seg_off))

    def to_granges(self, gr):
        """The junctions as genomic ranges: ``(GRanges, columns)``.  ``gr``: the ranges of the call.  One range per junction
        -- the intron, 1-based, on its range's sequence and with its range's strand (a range's strand mirrors nothing: the
        coordinates are genomic) --, in the caller's range order and ascending inside each; ``columns``: ``range`` (index
        into ``gr``), ``count`` and ``max_anchor`` in the same order."""
        rng = self._range_of(gr)
        out = GRanges([gr.seqnames[i] for i in rng], self.start, width=self.end - self.start + 1, strand=[gr.strand[i] for i in rng])
        return out, dict(range=rng, count=self.count, max_anchor=self.max_anchor)

    def to_bed(self, path, gr):
        """Write the junctions as BED6: ``chrom  chromStart  chromEnd  range{i}_{j}  count  strand`` -- the intron in 0-based
        half-open coordinates, ``i`` the range and ``j`` the junction inside it, the score the supporting reads (strands
        summed); the strand is ``.``, or with ss the strand most of the reads lie on (sense = the range's strand, ``*``
        counted as ``+``; a tie goes to sense).  Returns the number of lines."""
        rng = self._range_of(gr)
        j = np.arange(self.njunctions) - self.seg_off[rng] if len(rng) else rng
        if self.ss:
            sense = ["-" if gr.strand[i] == "-" else "+" for i in rng]
            strand = [s if c[0] >= c[1] else "+-"[s == "+"] for s, c in zip(sense, self.count.tolist())]
        else:
            strand = ["."] * len(rng)
        with open(path, "w") as f:
            f.write("".join(f"{gr.seqnames[i]}\t{a - 1}\t{b}\trange{i}_{k}\t{c}\t{s}\n"
                            for i, k, a, b, c, s in zip(rng.tolist(), j.tolist(), self.start.tolist(), self.end.tolist(),
                                                        self.support().tolist(), strand)))
        return len(rng)

    def __repr__(self):
        n = len(self)
        return (f"Junctions object of {n}{' strand-specific' if self.ss else ''} range{'s' if n != 1 else ''}, "
                f"{self.njunctions} junctions")


def _whole(value, name, lo, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be a whole number")
    if int(value) < lo or int(value) > hi:
        raise ValueError(f"{name} must lie between {lo} and {hi}")
    return int(value)


def from_native(seg_off, start, end, count, max_anchor, ss):
    """the library's columns (0-based first and last base, uint32 counts) as a Junctions"""
    return Junctions(seg_off, start.astype(np.int64) + 1, end.astype(np.int64) + 1, count, max_anchor, bool(ss))


def bamJunctions(bampath, gr=None, mapqual=0, filteredFlag=-1, minAnchor=0, ss=False, verbose=True):  # noqa: N802,N803
    """For each range, the splice junctions that lie within it with the reads that support them: a Junctions.

    ``gr=None``: one ``*`` range per sequence of the BAM's header, from base 1 to its length.  A junction belongs to a range
    that holds it whole (first and last base of the intron inside the range); overlapping ranges each report it.  A read
    counts if its mapping quality is at least ``mapqual``, it carries none of the ``filteredFlag`` bits (as in bamCoverage)
    and its anchor at the junction is at least ``minAnchor`` bases.  ``ss``: counts split into the reads on the range's
    strand and those on the other one."""
    mq = _whole(mapqual, "mapqual", 0, 255)
    ff = _whole(filteredFlag, "filteredFlag", -1, 0xFFFF)
    anchor = _whole(minAnchor, "minAnchor", 0, 2**31 - 1)
    if not isinstance(ss, (bool, np.bool_)):
        raise ValueError("ss must be True or False")
    if gr is not None:
        _w._check_gr(gr)
    path = os.path.expanduser(str(bampath))
    if verbose:
        _w._print_sentence(bampath)
    if gr is None:
        from .bamio import BamFile
        bam = BamFile(path)
        try:
            gr = GRanges(list(bam.ref_names), np.ones(len(bam.ref_names), dtype=np.int64), width=np.asarray(bam.ref_len, dtype=np.int64))
        finally:
            bam.close()
    head = _w._head(path, gr, ())
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.bsig_junctions(*head[:8], mq, 0, ff, anchor, int(bool(ss)), _w._dev(None), C.byref(h)))
    from .device import take_junctions
    return from_native(*take_junctions(lib, h, bool(ss)), bool(ss))
