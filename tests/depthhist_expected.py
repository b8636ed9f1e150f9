"""The expected side of the depth histogram tests (a helper, not a conftest): the definition, literally -- the C oracle's
per-base cells of all ranges (bamCoverage's, or bamProfile's with binsize 1 and shift 0), np.bincount of min(cell, V),
then [number of cells, sum of the cells].  Never the GPU plan.  `restated` says the cells directly in numpy (difference
array + cumsum, bincount of the 5' ends), for the CPU tests."""
import numpy as np

from crosscorr_expected import merge_sorted, oracle_reads  # noqa: F401  (shared column helpers)
from fragsizes_expected import planted  # noqa: F401


def cells(cols_or_oracle, rg, signal, ss, **params):
    """all cells of all ranges, int64, in the oracle's order; params: the oracle's tlen_filter / mapqual / requiredF /
    filteredF and tspan (coverage) or pe_mid (ends)"""
    from oracle import oracle_c
    orc = cols_or_oracle if hasattr(cols_or_oracle, "c") else oracle_reads(cols_or_oracle)
    if len(rg["len"]) == 0:
        return np.zeros(0, np.int64)
    if signal == "coverage":
        assert not ss
        out, _ = oracle_c.coverage_core(orc, rg, **params)
    else:
        out, _ = oracle_c.pileup_core(orc, rg, binsize=1, shift=0, ss=bool(ss), **params)
    return np.asarray(out, np.int64)


def from_cells(c, max_value):
    c = np.asarray(c, np.int64)
    hist = np.bincount(np.minimum(c, max_value), minlength=max_value + 1).astype(np.int64)
    return np.concatenate([hist, [c.size, c.sum()]]).astype(np.int64)


def expected(cols_or_oracle, rg, signal, ss, max_value, **params):
    """max_value + 1 rows, then the two moments"""
    return from_cells(cells(cols_or_oracle, rg, signal, ss, **params), max_value)


def restated_cells(cols, rg, signal, ss, mapqual=0):
    """the cells without the oracle: per range a difference array and its cumsum (coverage), or a bincount of the 5' ends
    per strand (ends); no template-length rule.  A '-' range is mirrored, which permutes its cells and swaps its strands."""
    ref_off = np.asarray(cols["ref_off"], np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    pos, end = np.asarray(cols["pos"], np.int64), np.asarray(cols["end"], np.int64)
    flag, mapq = np.asarray(cols["flag"], np.int64), np.asarray(cols["mapq"], np.int64)
    neg = (flag & 16) != 0
    ok = mapq >= mapqual
    out = []
    for r, lo, w in zip(rg["rid"], rg["loc"], rg["len"]):
        lo, w = int(lo), int(w)
        if w <= 0:
            continue
        m = ok & (rid == r)
        if signal == "coverage":
            a, b = np.maximum(pos[m] - lo, 0), np.minimum(end[m] - lo, w - 1)
            keep = a <= b
            d = np.zeros(w + 1, np.int64)
            np.add.at(d, a[keep], 1)
            np.add.at(d, b[keep] + 1, -1)
            out.append(np.cumsum(d)[:w])
        else:
            p5 = np.where(neg[m], end[m], pos[m]) - lo
            inside = (p5 >= 0) & (p5 < w)
            plus = np.bincount(p5[inside & ~neg[m]], minlength=w).astype(np.int64)
            minus = np.bincount(p5[inside & neg[m]], minlength=w).astype(np.int64)
            out.append(np.concatenate([plus, minus]) if ss else plus + minus)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def n_cells(rg, ss):
    """the plan-independent cell count: the widths, twice with strands"""
    return int(np.maximum(np.asarray(rg["len"], np.int64), 0).sum()) * (2 if ss else 1)
