"""bamSites: at which bases do the reads disagree with the reference, or with each other?  The candidate stage of VarScan, of
``bcftools mpileup | call`` and of ``deepSNV``, and the filter everybody writes over ``Rsamtools::pileup``: SNV and deletion
candidates, het sites for allele-specific work, sample-identity fingerprints, editing sites.  The cells are those of
``bamNucleotides`` -- the same reads, the same base filter, a ``-`` range reversed and complemented -- but they are judged on
the GPU where they are counted (csrc/sites.hip), and only the sites come back: ``bamSites(...)`` equals the same filter applied
to ``bamNucleotides(...)``.

For a base with the six counts ``A C G T N -`` (strands summed) and their sum D: the BASE channel b is the reference's
(``ref``; a base whose reference is not one of ACGT is never a site) or, without ``ref``, the first channel with the most
counts; the ALT channel a is the first with the most counts among ``A C G T`` -- and ``-`` with ``deletions`` --, b excluded
(N is never an allele).  The base is a site iff D >= ``minDepth``, count[a] >= ``minAlt`` and count[a] / D >= ``minFraction``
(decided in whole numbers: count[a] * den >= num * D).  Insertions, de-duplication of overlapping mates, a reference read
from FASTA and genotype likelihoods are not built.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction

import numpy as np

from . import _lib
from . import wrappers as _w
from .nucleotides import CHANNELS, _whole

MAX_DENOMINATOR = 1 << 20
REF_N = 4


class AlleleSites:
    """The sites of n ranges, read-only.  Range i owns entries ``seg_off[i] .. seg_off[i + 1]`` of ``pos`` (the base's index
    in the range, 0-based, in the range's reading direction -- a ``-`` range counts from its right end --, ascending inside a
    range), ``base`` and ``alt`` (indices into ``channels``) and ``counts`` (int32 ``(n, 6)``, or with ss ``(n, 2, 6)``: the
    reads on the range's strand and those on the other one; a ``-`` range's counts are complemented, as the range reads)."""

    channels = CHANNELS
    FIELDS = ("pos", "base", "alt", "counts")

    def __init__(self, seg_off, pos, base, alt, counts, ss=False):
        if not isinstance(ss, (bool, np.bool_)):
            raise ValueError("invalid ss slot")
        self.ss = bool(ss)
        self.seg_off = np.array(seg_off, dtype=np.int64)
        self.pos = np.array(pos, dtype=np.int64)
        self.base = np.array(base, dtype=np.int64)
        self.alt = np.array(alt, dtype=np.int64)
        self.counts = np.array(counts, dtype=np.int32)
        n = len(self.pos)
        if self.seg_off.ndim != 1 or len(self.seg_off) < 1 or self.seg_off[0] != 0 or np.any(np.diff(self.seg_off) < 0) \
                or self.seg_off[-1] != n:
            raise ValueError("seg_off must hold one entry per range and one more, from 0 to the number of sites")
        if n == 0:
            self.counts = self.counts.reshape((0, 2, 6) if self.ss else (0, 6))
        if self.counts.shape != ((n, 2, 6) if self.ss else (n, 6)) or any(a.shape != (n,) for a in (self.pos, self.base, self.alt)):
            raise ValueError("the site arrays do not fit each other")
        if n and (np.any(self.pos < 0) or np.any(self.counts < 0) or np.any(self.base < 0) or np.any(self.base > 5)
                  or np.any(self.alt < 0) or np.any(self.alt > 5) or np.any(self.alt == self.base)):
            raise ValueError("a site needs a position and counts that are not negative and two different channels")
        for a in (self.seg_off, self.pos, self.base, self.alt, self.counts):
            a.setflags(write=False)

    def __len__(self):
        return len(self.seg_off) - 1

    @property
    def nsites(self):
        """total number of sites"""
        return int(self.seg_off[-1])

    def __getitem__(self, i):
        """the sites of range i: a dict of array views (pos, base, alt, counts)"""
        n = len(self)
        if not isinstance(i, (int, np.integer)):
            raise TypeError("index an AlleleSites with one integer")
        if i < -n or i >= n:
            raise IndexError("range index out of range")
        i = int(i) % n
        a, b = int(self.seg_off[i]), int(self.seg_off[i + 1])
        return {f: getattr(self, f)[a:b] for f in self.FIELDS}

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def range_index(self):
        """the range of every site (int64)"""
        return np.repeat(np.arange(len(self), dtype=np.int64), np.diff(self.seg_off))

    def summed(self):
        """``(n, 6)`` int64: the counts of every site, strands summed"""
        c = self.counts.astype(np.int64)
        return c.sum(axis=1) if self.ss else c

    def depth(self):
        """reads (deletions included) at every site, strands summed (int64)"""
        return self.summed().sum(axis=1)

    def alt_count(self):
        """reads that show the alt channel at every site, strands summed (int64)"""
        return self.summed()[np.arange(self.nsites), self.alt]

    def alt_fraction(self):
        """alt_count / depth (float64)"""
        return self.alt_count() / np.maximum(self.depth(), 1)

    def _range_of(self, gr):
        _w._check_gr(gr)
        if len(gr) != len(self):
            raise ValueError("gr must be the ranges the sites were found for")
        rng = self.range_index()
        if len(rng) and np.any(self.pos >= np.asarray(gr.width, dtype=np.int64)[rng]):
            raise ValueError("gr must be the ranges the sites were found for")
        return rng

    def genomic_pos(self, gr):
        """the 1-based genomic position of every site (int64): a ``-`` range's positions count down from its last base"""
        rng = self._range_of(gr)
        start = np.asarray(gr.start, dtype=np.int64)[rng]
        width = np.asarray(gr.width, dtype=np.int64)[rng]
        minus = np.asarray([s == "-" for s in gr.strand], dtype=bool)[rng] if len(rng) else np.zeros(0, dtype=bool)
        return np.where(minus, start + width - 1 - self.pos, start + self.pos).astype(np.int64)

    def to_table(self, gr):
        """One row per site: a dict of columns ``seqnames`` (list), ``pos`` (1-based genomic position), ``range`` (index into
        ``gr``), ``A C G T N -`` (int64, strands summed; a ``-`` range's counts stay complemented, as the range reads them) and
        ``ref`` and ``alt`` (lists of channel names: the base and the alt channel).  ``gr``: the ranges of the call."""
        rng = self._range_of(gr)
        c = self.summed()
        out = dict(seqnames=[gr.seqnames[i] for i in rng.tolist()], pos=self.genomic_pos(gr), range=rng)
        out.update({ch: c[:, k] for k, ch in enumerate(CHANNELS)})
        out["ref"] = [CHANNELS[k] for k in self.base.tolist()]
        out["alt"] = [CHANNELS[k] for k in self.alt.tolist()]
        return out

    def to_bed(self, path, gr):
        """Write the sites as BED6: ``chrom  chromStart  chromEnd  base>alt  score  strand`` -- the base in 0-based half-open
        coordinates, the name the two channels as the range reads them, the score the alt fraction in parts per thousand
        (rounded down), the strand the range's (``.`` for ``*``).  Returns the number of lines."""
        rng = self._range_of(gr)
        at = self.genomic_pos(gr)
        score = (self.alt_count() * 1000) // np.maximum(self.depth(), 1)
        with open(path, "w") as f:
            f.write("".join(f"{gr.seqnames[i]}\t{p - 1}\t{p}\t{CHANNELS[b]}>{CHANNELS[a]}\t{s}\t{'.' if gr.strand[i] == '*' else gr.strand[i]}\n"
                            for i, p, b, a, s in zip(rng.tolist(), at.tolist(), self.base.tolist(), self.alt.tolist(), score.tolist())))
        return len(rng)

    def __repr__(self):
        n = len(self)
        return (f"AlleleSites object of {n}{' strand-specific' if self.ss else ''} range{'s' if n != 1 else ''}, "
                f"{self.nsites} sites")


def from_native(seg_off, pos, alleles, counts, ss):
    """the library's columns (alleles = base | alt << 8) as an AlleleSites"""
    alleles = np.asarray(alleles)
    return AlleleSites(seg_off, pos, alleles & 0xFF, (alleles >> 8) & 0xFF, counts, bool(ss))


_CODE = np.full(256, REF_N, dtype=np.uint8)
for _k, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _k


def fraction_of(value, name="minFraction"):
    """``(num, den)`` of a float, an int or a Fraction between 0 and 1: ``Fraction(str(x)).limit_denominator(2^20)``"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating, Fraction)):
        raise ValueError(f"{name} must be a number")
    try:
        f = Fraction(str(value)).limit_denominator(MAX_DENOMINATOR)
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"{name} must be a finite number") from None
    if f < 0 or f > 1:
        raise ValueError(f"{name} must lie between 0 and 1")
    return int(f.numerator), int(f.denominator)


def ref_codes(ref, width):
    """one str or bytes per range, of the range's width -> the channel codes of all of them (uint8: ACGT in either case 0 .. 3,
    everything else 4)"""
    if isinstance(ref, (str, bytes)) or not hasattr(ref, "__len__"):
        raise ValueError("ref must hold one str or bytes per range")
    if len(ref) != len(width):
        raise ValueError("ref must hold one sequence per range")
    parts = []
    for i, (s, w) in enumerate(zip(ref, width)):
        if isinstance(s, str):
            try:
                s = s.encode("ascii")
            except UnicodeEncodeError:
                raise ValueError(f"ref[{i}] holds characters outside ASCII") from None
        if not isinstance(s, (bytes, bytearray)):
            raise ValueError("ref must hold one str or bytes per range")
        if len(s) != int(w):
            raise ValueError(f"ref[{i}] has {len(s)} bases, its range {int(w)}")
        parts.append(_CODE[np.frombuffer(bytes(s), dtype=np.uint8)])
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint8)


def take_sites(lib, handle, ss):
    """a bsig_sites_result handle -> (seg_off, pos, alleles, counts); the handle is freed"""
    try:
        n_seg, n = int(lib.bsig_sites_result_n_ranges(handle)), int(lib.bsig_sites_result_n_sites(handle))
        out = [np.empty(n_seg + 1, dtype=np.int64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32),
               np.empty((n, 2, 6) if ss else (n, 6), dtype=np.int32)]
        _lib.check(lib.bsig_sites_result_copy(handle, *[a.ctypes.data if a.size else None for a in out]))
    finally:
        lib.bsig_sites_result_free(handle)
    return tuple(out)


def bamSites(bampath, gr, ref=None, minDepth=10, minAlt=2, minFraction=0.2, deletions=True, mapqual=0,  # noqa: N802,N803
             filteredFlag=-1, minBaseQuality=0, ss=False, verbose=True):
    """For each range, the bases at which the reads disagree with ``ref`` -- or, without it, with each other: an AlleleSites.

    ``ref``: one ``str`` or ``bytes`` per range, of the range's width, in the range's own reading direction (for a ``-`` range
    the reverse complement, as ``getSeq(genome, gr)`` gives it); case does not matter, anything but ACGT counts as N and is
    never a site.  A base is a site if at least ``minDepth`` reads count there, at least ``minAlt`` of them show the alt
    channel and they are at least ``minFraction`` of all (a float, an int or a ``Fraction``).  ``deletions``: may the alt be a
    deletion?  The reads and bases that count are those of ``bamNucleotides`` (``mapqual``, ``filteredFlag``,
    ``minBaseQuality``); ``ss`` splits the reported counts by strand and changes no decision."""
    depth = _whole(minDepth, "minDepth", 1, 2**31 - 1)
    alt = _whole(minAlt, "minAlt", 1, 2**31 - 1)
    num, den = fraction_of(minFraction)
    if not isinstance(deletions, (bool, np.bool_)):
        raise ValueError("deletions must be True or False")
    mq = _whole(mapqual, "mapqual", 0, 255)
    ff = _whole(filteredFlag, "filteredFlag", -1, 0xFFFF)
    bq = _whole(minBaseQuality, "minBaseQuality", 0, 93)
    if not isinstance(ss, (bool, np.bool_)):
        raise ValueError("ss must be True or False")
    _w._check_gr(gr)
    codes = None if ref is None else ref_codes(ref, gr.width)
    path = os.path.expanduser(str(bampath))
    if verbose:
        _w._print_sentence(bampath)
    head = _w._head(path, gr, ())
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.bsig_sites(*head[:8], mq, 0, ff, bq, int(bool(ss)), None if codes is None else codes.ctypes.data, depth, alt, num, den,
                              0x2F if deletions else 0x0F, _w._dev(None), C.byref(h)))
    return from_native(*take_sites(lib, h, bool(ss)), bool(ss))
