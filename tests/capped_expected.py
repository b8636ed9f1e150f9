"""The expected side of the capped signals (keepDup; a helper, not a conftest): the definition, literally, and never the
GPU plan.  The C oracle's per-base, per-strand 5'-end cells (pileup_core with binsize 1 and ss) are capped with
np.minimum(., k); the ends form sums them per bin with np.add.reduceat and folds the strands last; the coverage form takes
the same capped cells over the range widened by L - 1 bases on both sides -- zeros for bases below 0 -- and the two window
sums of the definition, in range orientation:
    cell x = sum of c_sense[p], p = x - L + 1 .. x,  +  sum of c_anti[p], p = x .. x + L - 1."""
import numpy as np

from crosscorr_expected import merge_sorted, oracle_reads  # noqa: F401  (shared column helpers)
from fragsizes_expected import planted  # noqa: F401


def _orc(cols_or_oracle):
    return cols_or_oracle if hasattr(cols_or_oracle, "c") else oracle_reads(cols_or_oracle)


def stranded_cells(cols_or_oracle, rg, shift=0, **filters):
    """per range the (2, w) int64 matrix of its per-base 5'-end cells, rows sense and antisense, uncapped"""
    from oracle import oracle_c
    n = len(rg["len"])
    if n == 0:
        return []
    out, off = oracle_c.pileup_core(_orc(cols_or_oracle), rg, binsize=1, shift=shift, ss=True, **filters)
    return [out[off[i]:off[i + 1]].astype(np.int64).reshape(-1, 2).T for i in range(n)]


def _bins(row, binsize):
    """the sums of a row over bins of binsize cells (binsize <= 0: the one bin of bamCount, which a range without width has too)"""
    if binsize <= 0:
        return np.asarray([row.sum()], np.int64)
    return np.add.reduceat(row, np.arange(0, len(row), binsize)) if len(row) else np.zeros(0, np.int64)


def _lay(rows2, binsize, ss):
    """one range's cells in the flat layout: 2 * bin + antisense with strands, the strands added without"""
    s, a = _bins(rows2[0], binsize), _bins(rows2[1], binsize)
    return np.stack([s, a]).T.reshape(-1) if ss else s + a


def _flat(parts):
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int64), off


def ends_from_cells(cells, k, binsize=1, ss=False):
    """(flat int64 cells, offsets) from stranded_cells' matrices: capped first, binned second, the strands added last"""
    return _flat([_lay(np.minimum(c, k), binsize, ss) for c in cells])


def ends(cols_or_oracle, rg, k, binsize=1, ss=False, shift=0, **filters):
    return ends_from_cells(stranded_cells(cols_or_oracle, rg, shift=shift, **filters), k, binsize, ss)


def coverage(cols_or_oracle, rg, k, L, binsize=1, ss=False, **filters):
    """(flat int64 cells, offsets) of the coverage of the kept reads resized to L bases"""
    L = int(L)
    loc, ln, strand = (np.asarray(rg[key], np.int64) for key in ("loc", "len", "strand"))
    # (widened by L - 1 on both sides, the left end clipped at base 0: lead may be negative for a range that begins below 0)
    lo = np.maximum(loc - (L - 1), 0)
    lead = loc - lo
    wide = dict(rid=np.asarray(rg["rid"], np.int32), loc=lo.astype(np.int32),
                len=np.where(ln > 0, np.maximum(lead + ln + L - 1, 0), 0).astype(np.int32), strand=np.asarray(rg["strand"], np.int32))
    parts = []
    for i, c in enumerate(stranded_cells(cols_or_oracle, wide, **filters)):
        w = int(ln[i])
        if w <= 0:
            parts.append(np.zeros(0, np.int64))
            continue
        c = np.minimum(c, k)
        # zeros for the bases below 0: in front of a '+' range's row, behind a mirrored '-' range's
        pad = np.zeros((2, w + 2 * L - 2 - c.shape[1]), np.int64)
        c = np.concatenate([c, pad], axis=1) if strand[i] < 0 else np.concatenate([pad, c], axis=1)
        cs = np.concatenate([np.zeros((2, 1), np.int64), np.cumsum(c, axis=1)], axis=1)
        x = np.arange(w)
        sense = cs[0, x + L] - cs[0, x]                      # p = x - L + 1 .. x, at index p + L - 1
        anti = cs[1, x + 2 * L - 1] - cs[1, x + L - 1]       # p = x .. x + L - 1
        # a cell below base 0 is covered by nothing: no read lies there
        below = (loc[i] + (w - 1 - x if strand[i] < 0 else x)) < 0
        sense[below] = 0
        anti[below] = 0
        parts.append(_lay(np.stack([sense, anti]), binsize, ss))
    return _flat(parts)
