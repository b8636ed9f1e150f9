"""The expected side of the V-plot tests (a helper, not a conftest): the definition, literally -- per non-empty row band
one bamProfile of the C oracle (binsize, unstranded, unshifted, requiredF 66, the position rule) with the band as its tlen
filter, summed over the ranges.  Never the GPU plan.  `restated` is the same thing said directly in numpy (filter,
position, mirror, np.add.at), for the CPU tests."""
import numpy as np

from crosscorr_expected import merge_sorted, oracle_reads  # noqa: F401  (shared column helpers)
from fragsizes_expected import planted  # noqa: F401


def shape(rg, tf, lenbin, binsize):
    w = int(rg["len"][0]) if len(rg["len"]) else 0
    return int(tf[1]) // int(lenbin) + 1, (w + int(binsize) - 1) // int(binsize) if w > 0 else 0


def expected(cols, rg, tf, lenbin, binsize, midpoint, **filters):
    """counts[r, j] = sum_i bamProfile(rg[i], binsize, ss False, shift 0, requiredF 66, pe_mid = midpoint, tlen_filter =
    row r's band)[j]; filters: the oracle's mapqual / filteredF.  cols: columns or the oracle's reads."""
    from oracle import oracle_c
    orc = cols if hasattr(cols, "c") else oracle_reads(cols)
    rows, n_cols = shape(rg, tf, lenbin, binsize)
    counts = np.zeros((rows, n_cols), np.int64)
    if n_cols == 0:
        return counts
    for r in range(rows):
        band = (max(int(tf[0]), r * lenbin), min(int(tf[1]), (r + 1) * lenbin - 1))
        if band[0] > band[1]:
            continue
        out, _ = oracle_c.pileup_core(orc, rg, binsize=int(binsize), shift=0, ss=False, requiredF=66, pe_mid=bool(midpoint),
                                      tlen_filter=band, **filters)
        counts[r] = np.asarray(out, np.int64).reshape(len(rg["len"]), n_cols).sum(axis=0)
    return counts


def restated(cols, rg, tf, lenbin, binsize, midpoint, mapqual=0, filteredF=-1):
    """filter, position, mirror, np.add.at on (a // lenbin, rel // binsize) per range (read_rejected:
    oracle/bamsignals_oracle.c:91-102)"""
    ref_off = np.asarray(cols["ref_off"], np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    pos, end = np.asarray(cols["pos"], np.int64), np.asarray(cols["end"], np.int64)
    flag, mapq = np.asarray(cols["flag"], np.int64), np.asarray(cols["mapq"], np.int64)
    a = np.abs(np.asarray(cols["tlen"], np.int64))
    nf = ~flag
    ok = (mapq >= mapqual) & ((66 & nf) == 0) & ((np.int64(filteredF) & nf & 0xFFFFFFFF) != 0) & (a >= tf[0]) & (a <= tf[1])
    neg = (flag & 16) != 0
    off = a // 2 if midpoint else 0
    p5 = np.where(neg, end - off, pos + off)
    counts = np.zeros(shape(rg, tf, lenbin, binsize), np.int64)
    for r, lo, w, s in zip(rg["rid"], rg["loc"], rg["len"], rg["strand"]):
        m = ok & (rid == r) & (p5 >= lo) & (p5 < int(lo) + int(w))
        rel = p5[m] - int(lo)
        if s < 0:
            rel = int(w) - 1 - rel
        np.add.at(counts, (a[m] // lenbin, rel // binsize), 1)
    return counts


def frag_marginal(cols, rg, tf, lenbin, midpoint, mapqual=0, filteredF=-1):
    """fragsizes_expected.restated: what the rows must sum to"""
    import fragsizes_expected as fe
    return fe.restated(cols, rg, tf, lenbin, midpoint, mapqual=mapqual, filteredF=filteredF)


def profile_marginal(cols, rg, tf, binsize, midpoint, **filters):
    """the oracle's one bamProfile with the whole filter, summed over the ranges: what the columns must sum to"""
    from oracle import oracle_c
    orc = cols if hasattr(cols, "c") else oracle_reads(cols)
    n_cols = shape(rg, tf, 1, binsize)[1]
    if n_cols == 0:
        return np.zeros(0, np.int64)
    out, _ = oracle_c.pileup_core(orc, rg, binsize=int(binsize), shift=0, ss=False, requiredF=66, pe_mid=bool(midpoint),
                                  tlen_filter=tuple(int(x) for x in tf), **filters)
    return np.asarray(out, np.int64).reshape(len(rg["len"]), n_cols).sum(axis=0)
