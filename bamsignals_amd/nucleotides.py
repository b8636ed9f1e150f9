"""bamNucleotides: what do the reads SAY at every base of a range?  For each base the number of reads that show an A, a C, a G,
a T, something else (``N``: ``=``, an IUPAC ambiguity code, or a base the record does not hold) or a deletion there: the
nucleotide table of ``Rsamtools::pileup``, ``bam-readcount``, ``deepSNV::bam2R`` and the count columns of ``samtools mpileup``
-- allele fractions at known SNPs, mismatch and error profiles, a consensus, editing and conversion rates all start from it.
Counted on the GPU (csrc/nucleotides.hip) from the base table that the file's reads with bases keep; no CIGAR is walked on the
host.

A read takes part if it is mapped (flag 0x4 clear), its mapping quality is at least ``mapqual`` and it carries none of the
``filteredFlag`` bits (as in bamCoverage).  Its CIGAR places the bases: ``M = X`` put query bases on reference bases, ``I`` and
``S`` skip query bases, ``D`` counts one deletion per reference base, ``N`` skips reference bases, ``H`` and ``P`` do nothing.  A
base counts if its quality is at least ``minBaseQuality``; a missing quality (``QUAL`` = ``*``) passes every threshold, a
deletion has none and always counts.  Insertion counts, counts by position in the read, de-duplication of overlapping mates
and ``binsize`` > 1 are not built.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from . import wrappers as _w

CHANNELS = ("A", "C", "G", "T", "N", "-")


class NucleotideCounts:
    """The nucleotide counts of n ranges, read-only.  ``nc[i]`` is an int32 array ``(6, width)`` -- rows ``channels`` -- or,
    with ss, ``(2, 6, width)``: the reads on the range's strand (``*`` counted as ``+``) and those on the other one.  A ``-``
    range reads 5' -> 3' on its own strand: positions reversed, channels complemented (A <-> T, C <-> G)."""

    channels = CHANNELS

    def __init__(self, arrays, ss=False):
        if not isinstance(ss, (bool, np.bool_)):
            raise ValueError("invalid ss slot")
        self.ss = bool(ss)
        lead = (2, 6) if self.ss else (6,)
        self._arrays = []
        for a in arrays:
            a = np.asarray(a)
            if a.dtype != np.int32 or a.shape[:-1] != lead:
                raise ValueError(f"every range needs an int32 array of shape {lead + ('width',)}")
            if a.flags.writeable:
                a = a.copy()
                a.setflags(write=False)
            self._arrays.append(a)

    def __len__(self):
        return len(self._arrays)

    def __getitem__(self, i):
        n = len(self)
        if not isinstance(i, (int, np.integer)):
            raise TypeError("index a NucleotideCounts with one integer")
        if i < -n or i >= n:
            raise IndexError("range index out of range")
        return self._arrays[int(i) % n]

    def __iter__(self):
        return iter(self._arrays)

    def counts(self, i):
        """``(6, width)`` int64: the counts of range i, strands summed"""
        a = self[i].astype(np.int64)
        return a.sum(axis=0) if self.ss else a

    def depth(self, i):
        """reads (deletions included) per base of range i: the sum over the channels and, with ss, the strands (int64)"""
        return self.counts(i).sum(axis=0)

    def major(self, i):
        """the index into ``channels`` of the channel with the most counts per base, the first on a tie; -1 where nothing
        counts"""
        c = self.counts(i)
        return np.where(c.sum(axis=0) > 0, np.argmax(c, axis=0), -1).astype(np.int64)

    def fraction(self, i, channel):
        """the share of ``channel`` (a name of ``channels`` or its index) in the depth per base: float64, NaN where nothing
        counts"""
        k = CHANNELS.index(channel) if isinstance(channel, str) else int(channel)
        if k < 0 or k >= len(CHANNELS):
            raise ValueError("no such channel")
        c = self.counts(i)
        d = c.sum(axis=0)
        return np.where(d > 0, c[k] / np.maximum(d, 1), np.nan).astype(np.float64)

    def to_table(self, gr):
        """One row per base with a count: a dict of columns ``seqnames`` (list), ``pos`` (1-based genomic position), ``range``
        (index into ``gr``) and ``A C G T N -`` (int64, strands summed; a ``-`` range's counts stay complemented, as the range
        reads them).  ``gr``: the ranges of the call."""
        _w._check_gr(gr)
        if len(gr) != len(self) or any(int(w) != a.shape[-1] for w, a in zip(gr.width, self._arrays)):
            raise ValueError("gr must be the ranges the nucleotides were counted for")
        names, pos, rng, cnt = [], [], [], []
        for i in range(len(self)):
            c = self.counts(i)
            j = np.flatnonzero(c.sum(axis=0) > 0)
            at = int(gr.start[i]) + int(gr.width[i]) - 1 - j if gr.strand[i] == "-" else int(gr.start[i]) + j
            names += [gr.seqnames[i]] * len(j)
            pos.append(at.astype(np.int64)); rng.append(np.full(len(j), i, dtype=np.int64)); cnt.append(c[:, j])
        cat = np.concatenate(cnt, axis=1) if cnt else np.zeros((6, 0), dtype=np.int64)
        out = dict(seqnames=names, pos=np.concatenate(pos) if pos else np.zeros(0, dtype=np.int64),
                   range=np.concatenate(rng) if rng else np.zeros(0, dtype=np.int64))
        out.update({ch: cat[k] for k, ch in enumerate(CHANNELS)})
        return out

    def __repr__(self):
        n = len(self)
        return f"NucleotideCounts object of {n}{' strand-specific' if self.ss else ''} range{'s' if n != 1 else ''}"


def _whole(value, name, lo, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be a whole number")
    if int(value) < lo or int(value) > hi:
        raise ValueError(f"{name} must lie between {lo} and {hi}")
    return int(value)


def bamNucleotides(bampath, gr, mapqual=0, filteredFlag=-1, minBaseQuality=0, ss=False, verbose=True):  # noqa: N802,N803
    """For each range, the A / C / G / T / N / deletion counts of every base: a NucleotideCounts.

    A read counts if it is mapped, its mapping quality is at least ``mapqual`` and it carries none of the ``filteredFlag`` bits
    (as in bamCoverage); a base counts if its quality is at least ``minBaseQuality`` (0 .. 93; a missing quality always
    passes).  ``ss``: counts split into the reads on the range's strand and those on the other one.  With
    ``minBaseQuality=0`` the channels of a base add up to ``bamCoverage(splice=True)`` there."""
    mq = _whole(mapqual, "mapqual", 0, 255)
    ff = _whole(filteredFlag, "filteredFlag", -1, 0xFFFF)
    bq = _whole(minBaseQuality, "minBaseQuality", 0, 93)
    if not isinstance(ss, (bool, np.bool_)):
        raise ValueError("ss must be True or False")
    _w._check_gr(gr)
    path = os.path.expanduser(str(bampath))
    if verbose:
        _w._print_sentence(bampath)
    head = _w._head(path, gr, ())
    lib = _lib.load()
    n = len(gr)
    off = np.zeros(n + 1, dtype=np.int64)
    cells = int(lib.bsig_nucleotides_cells(n, head.width.ctypes.data, int(bool(ss)), off.ctypes.data))
    out = np.zeros(max(cells, 1), dtype=np.int32)
    _lib.check(lib.bsig_nucleotides(*head[:8], mq, 0, ff, bq, int(bool(ss)), _w._dev(None), out.ctypes.data))
    from .device import split_nucleotides
    return NucleotideCounts(split_nucleotides(out, off, head.width, bool(ss)), bool(ss))
