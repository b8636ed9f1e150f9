"""bamGeneCounts: how many reads does each gene have?  The table every differential-expression analysis starts from
(``htseq-count -m union``, featureCounts' default, ``summarizeOverlaps(exonsBy(txdb, "gene"), mode="Union")``), counted on
the GPU (csrc/genecounts.hip) from the read table that the file's spliced reads keep -- the same resident set
``bamCoverage(splice=True)`` and ``bamJunctions`` use --; only one int64 per gene and five more come back.

The rule.  A read's blocks are what ``bamCoverage(splice=True)`` covers: its span minus its ``N`` gaps.  Its strand is ``-`` if
it carries 0x10, else ``+``, and the other one if it is a second mate (0x1 and 0x80).  A feature matches the read always
(``"unstranded"``), if it is ``*`` or on the read's strand (``"forward"``), or if it is ``*`` or on the other strand
(``"reverse"``).  In this order: an unmapped read (0x4) is ``unmapped``; a read below ``mapqual`` or with every
``filteredFlag`` bit (or, with ``paired_end="filter"``, not the first mate of a proper pair) is ``filtered``; then with H =
the genes that have a matching feature on the read's sequence sharing at least one base with at least one block, the read is
``no_feature`` (H empty), ``assigned`` to the one gene of H, or ``ambiguous`` (two or more).

Not built: ``intersection-strict`` / ``intersection-nonempty``; a minimum overlap (featureCounts ``--minOverlap`` /
``--fracOverlap``); multi-overlap counting (``-O``); counting a pair as ONE fragment from both mates' blocks (there are no
read names on the device: ``paired_end="filter"`` counts each proper pair once, by its first mate's blocks alone).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from . import wrappers as _w
from .granges import GRanges

STRAND_MODES = ("unstranded", "forward", "reverse")
SUMMARY_FIELDS = ("assigned", "ambiguous", "no_feature", "filtered", "unmapped")
TABLES = ("unstranded", "plus", "minus")


def _whole(value, name, lo, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be a whole number")
    if int(value) < lo or int(value) > hi:
        raise ValueError(f"{name} must lie between {lo} and {hi}")
    return int(value)


def strand_code(strand):
    """"unstranded" / "forward" / "reverse" (or the tuple of all three: the first) as the library's 0 / 1 / 2"""
    if isinstance(strand, (list, tuple)) and tuple(strand) == STRAND_MODES:
        strand = STRAND_MODES[0]
    if not isinstance(strand, str) or strand not in STRAND_MODES:
        raise ValueError("strand must be one of " + ", ".join(repr(s) for s in STRAND_MODES))
    return STRAND_MODES.index(strand)


class GeneModel:
    """Features that belong to genes, flattened once on the host (csrc/genemodel.h) and reusable for any number of files.

    ``gr``: the features (exons) as a GRanges; ``group``: one label per range saying which gene it belongs to.  Genes are
    ordered by first appearance (``.genes``).  Features may overlap, repeat, nest and come in any order; a feature of width
    0 takes part in nothing.  The model's sequences are the GRanges' own (``.seqlevels``), matched to a BAM by name."""

    def __init__(self, gr, group):
        _w._check_gr(gr)
        if isinstance(group, (str, bytes)) or not hasattr(group, "__len__"):
            raise ValueError("group must hold one label per range")
        if len(group) != len(gr):
            raise ValueError(f"group must hold one label per range: {len(group)} labels for {len(gr)} ranges")
        labels = list(dict.fromkeys(group.tolist() if isinstance(group, np.ndarray) else group))
        lut = {g: k for k, g in enumerate(labels)}
        gene = np.fromiter((lut[g] for g in (group.tolist() if isinstance(group, np.ndarray) else group)), dtype=np.int32, count=len(gr))
        levels, codes, start, width, strand = gr.flatten()
        self._init(codes, start.astype(np.int64) - 1, width, strand, gene, len(labels), len(levels), labels, levels)

    @classmethod
    def from_arrays(cls, rid, loc, length, strand, gene, n_genes, n_ref, genes=None, seqlevels=None):
        """The model from the library's own columns: reference index, 0-based ``loc``, ``length``, strand -1 / 0 / +1 and
        the gene index of every feature (what ``Reads.gene_counts`` needs: ``n_ref`` must be the reads')."""
        self = cls.__new__(cls)
        self._init(rid, loc, length, strand, gene, n_genes, n_ref, genes, seqlevels)
        return self

    def _init(self, rid, loc, length, strand, gene, n_genes, n_ref, genes, seqlevels):
        self._h = None
        cols = []
        for a, name in ((rid, "rid"), (loc, "loc"), (length, "length"), (strand, "strand"), (gene, "gene")):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"{name} must be a vector of whole numbers")
            if a.size and (a.min() < -2**31 or a.max() > 2**31 - 1):
                raise ValueError(f"{name} does not fit 32 bits")
            cols.append(np.ascontiguousarray(a, dtype=np.int32))
        n = len(cols[0])
        if any(len(a) != n for a in cols):
            raise ValueError("feature arrays differ in length")
        n_genes, n_ref = _whole(n_genes, "n_genes", 0, 2**31 - 8), _whole(n_ref, "n_ref", 0, 2**31 - 1)
        self.genes = tuple(range(n_genes)) if genes is None else tuple(genes)
        self.seqlevels = None if seqlevels is None else tuple(str(s) for s in seqlevels)
        if len(self.genes) != n_genes or (self.seqlevels is not None and len(self.seqlevels) != n_ref):
            raise ValueError("genes / seqlevels do not fit n_genes / n_ref")
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.bsig_gene_model_create(n, *[a.ctypes.data if a.size else None for a in cols], n_genes, n_ref, C.byref(h)))
        self._h = h
        self.n_features, self.n_genes, self.n_ref = n, n_genes, n_ref

    def __len__(self):
        return self.n_genes

    def n_segments(self, table="unstranded"):
        return int(self._lib.bsig_gene_model_n_segments(self._h, self._table(table)))

    @staticmethod
    def _table(table):
        if isinstance(table, str) and table in TABLES:
            return TABLES.index(table)
        if isinstance(table, (int, np.integer)) and not isinstance(table, (bool, np.bool_)) and 0 <= int(table) < 3:
            return int(table)
        raise ValueError("table must be one of " + ", ".join(repr(t) for t in TABLES) + " (or 0, 1, 2)")

    def segments(self, table="unstranded"):
        """The flattened table as arrays: ``dict(ref_off, start, end, value)`` -- the disjoint segments of sequence r are
        ``ref_off[r] .. ref_off[r + 1]``, ``start`` / ``end`` their first and last base (0-based), ``value`` the one gene
        active there (an index into ``.genes``) or -1 where two or more genes overlap.  ``"unstranded"``: all features;
        ``"plus"`` / ``"minus"``: those on that strand and the ``*`` ones."""
        t = self._table(table)
        n = int(self._lib.bsig_gene_model_n_segments(self._h, t))
        out = dict(ref_off=np.empty(self.n_ref + 1, dtype=np.int64), start=np.empty(n, dtype=np.int32), end=np.empty(n, dtype=np.int32),
                   value=np.empty(n, dtype=np.int32))
        _lib.check(self._lib.bsig_gene_model_copy_segments(self._h, t, *[a.ctypes.data if a.size else None for a in out.values()]))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bsig_gene_model_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __repr__(self):
        return (f"GeneModel of {self.n_genes} gene{'s' if self.n_genes != 1 else ''}, {self.n_features} features, "
                f"{self.n_segments()} segments")


class GeneCounts:
    """Reads per gene, read-only.  ``genes``: the labels; ``counts``: int64, one per gene -- ``(n_genes, n_files)`` where a
    list of files was counted --; ``summary``: int64 ``(5,)`` or ``(n_files, 5)`` in the order of ``SUMMARY_FIELDS``, also by
    name (``assigned``, ``ambiguous``, ``no_feature``, ``filtered``, ``unmapped``).  Every file's summary adds up to its
    reads, and its counts to ``assigned``."""

    def __init__(self, genes, counts, summary, files=None):
        self.genes = tuple(genes)
        self.counts = np.array(counts, dtype=np.int64)
        self.summary = np.array(summary, dtype=np.int64)
        many = self.counts.ndim == 2
        n_files = self.counts.shape[1] if many else 1
        if self.counts.ndim not in (1, 2) or self.counts.shape[0] != len(self.genes):
            raise ValueError("counts must hold one row per gene")
        if self.summary.shape != ((n_files, 5) if many else (5,)):
            raise ValueError("summary must hold five values per file")
        if np.any(self.counts < 0) or np.any(self.summary < 0):
            raise ValueError("counts are not negative")
        if not np.array_equal(self.counts.sum(axis=0), self.summary[..., 0]):
            raise ValueError("the genes' counts must add up to assigned")
        self.files = tuple(str(f) for f in files) if files is not None else tuple(f"file{k + 1}" for k in range(n_files))
        if len(self.files) != n_files:
            raise ValueError("files must name every column of counts")
        self.counts.setflags(write=False)
        self.summary.setflags(write=False)

    def __len__(self):
        return len(self.genes)

    def __getattr__(self, name):
        if name in SUMMARY_FIELDS:
            v = self.__dict__["summary"][..., SUMMARY_FIELDS.index(name)]
            return int(v) if v.ndim == 0 else v
        raise AttributeError(name)

    @property
    def n_reads(self):
        """the reads of every file: its summary added up"""
        v = self.summary.sum(axis=-1)
        return int(v) if v.ndim == 0 else v

    def assigned_fraction(self):
        """assigned / reads, per file (0 for a file without reads)"""
        total = np.asarray(self.summary.sum(axis=-1), dtype=np.float64)
        frac = np.divide(self.summary[..., 0], total, out=np.zeros_like(total), where=total > 0)
        return float(frac) if frac.ndim == 0 else frac

    def to_tsv(self, path):
        """Write the table as ``htseq-count`` does: one line per gene -- the label, then one count per file, tab-separated
        --, then the five summary lines ``__assigned`` .. ``__unmapped``.  Returns the number of lines."""
        counts = self.counts.reshape(len(self.genes), -1)
        summary = self.summary.reshape(-1, 5)
        lines = [f"{g}\t" + "\t".join(str(c) for c in row) for g, row in zip(self.genes, counts.tolist())]
        lines += [f"__{name}\t" + "\t".join(str(c) for c in summary[:, k].tolist()) for k, name in enumerate(SUMMARY_FIELDS)]
        with open(path, "w") as f:
            f.write("".join(line + "\n" for line in lines))
        return len(lines)

    def __repr__(self):
        n, k = len(self.genes), len(self.files)
        return (f"GeneCounts object of {n} gene{'s' if n != 1 else ''}, {k} file{'s' if k != 1 else ''}, "
                f"{int(self.summary[..., 0].sum())} of {int(self.summary.sum())} reads assigned")


def bamGeneCounts(bampath, gr, group=None, mapqual=0, filteredFlag=-1, strand=STRAND_MODES,  # noqa: N802,N803
                  paired_end=("ignore", "filter"), verbose=True):
    """Reads per gene: a GeneCounts.

    ``gr`` / ``group``: the features and their genes (see GeneModel), or ``gr`` a GeneModel made earlier and ``group=None``.
    ``bampath``: one path, or a list of paths -- the model is flattened once, ``counts`` then has one column per file and
    ``summary`` one row per file: the matrix DESeq2 and edgeR take.  Every sequence of the features must be one of the
    BAM's.  ``strand``: ``"unstranded"``, ``"forward"`` (the read lies on the gene's strand: ``htseq-count -s yes``,
    featureCounts ``-s 1``) or ``"reverse"`` (``-s reverse``, ``-s 2``).  ``paired_end="filter"`` counts each properly
    mapped pair once, by its first mate; ``"ignore"`` counts every read by itself.  The module's docstring has the rule."""
    mq = _whole(mapqual, "mapqual", 0, 255)
    ff = _whole(filteredFlag, "filteredFlag", -1, 0xFFFF)
    mode = strand_code(strand)
    pe = _w._match_arg(paired_end, ("ignore", "filter"), "paired.end")
    if not isinstance(verbose, (bool, np.bool_)):
        raise ValueError("verbose must be True or False")
    many = isinstance(bampath, (list, tuple))
    paths = [os.path.expanduser(str(p)) for p in (bampath if many else [bampath])]
    if many and not paths:
        raise ValueError("bampath holds no path")
    if isinstance(gr, GeneModel):
        if group is not None:
            raise ValueError("group must be None where gr is a GeneModel")
        model = gr
    else:
        _w._check_gr(gr)
        if group is None:
            raise ValueError("group must hold one label per range")
        model = GeneModel(gr, group)
    if model.seqlevels is None:
        raise ValueError("a GeneModel without sequence names (from_arrays without seqlevels) cannot be matched to a BAM")
    lib = _lib.load()
    names = (C.c_char_p * max(len(model.seqlevels), 1))(*[s.encode() for s in model.seqlevels])
    counts = np.zeros((len(paths), max(model.n_genes, 1)), dtype=np.int64)
    summary = np.zeros((len(paths), 5), dtype=np.int64)
    for k, path in enumerate(paths):
        if verbose:
            _w._print_sentence(path)
        _lib.check(lib.bsig_gene_counts(path.encode(), model._h, len(model.seqlevels), names, mq, _w.flagMask(pe), ff, mode, _w._dev(None),
                                        counts[k].ctypes.data, summary[k].ctypes.data))
    counts = counts[:, :model.n_genes].T
    if many:
        return GeneCounts(model.genes, counts, summary, files=paths)
    return GeneCounts(model.genes, counts[:, 0], summary[0], files=paths)
