"""The expected side of the per-range summary tests (a helper, not a conftest): the definition, literally -- the C oracle's
per-base cells (tests/depthhist_expected.py: cells), split per range with the oracle's layout, then sum, max, np.argmax
(first of ties) and count_nonzero(cells >= t) in numpy.  Never the GPU plan."""
import numpy as np

import depthhist_expected as de
from depthhist_expected import merge_sorted, oracle_reads, planted, restated_cells  # noqa: F401  (shared helpers)


def rows_of(cells, rg, ss):
    """the cells of every range as an (S, w) array: the oracle lays a strand-split range out as 2 * cell + antisense"""
    from oracle import oracle_c
    ln = np.asarray(rg["len"], np.int32)
    off = oracle_c.layout(ln, 1, bool(ss))
    assert int(off[-1]) == len(cells)
    S = 2 if ss else 1
    return [np.asarray(cells[off[i]:off[i + 1]], np.int64).reshape(-1, S).T for i in range(len(ln))]


def from_rows(rows, thresholds):
    """(n, S, 3 + K) int64 from the per-range (S, w) cell arrays"""
    K = len(thresholds)
    S = rows[0].shape[0] if rows else 1
    out = np.zeros((len(rows), S, 3 + K), np.int64)
    for i, c in enumerate(rows):
        if c.shape[1] == 0:
            out[i, :, 2] = -1
            continue
        out[i, :, 0] = c.sum(axis=1)
        out[i, :, 1] = c.max(axis=1)
        out[i, :, 2] = np.argmax(c, axis=1)
        for k, t in enumerate(thresholds):
            out[i, :, 3 + k] = np.count_nonzero(c >= t, axis=1)
    return out


def from_cells(cells, rg, ss, thresholds):
    if len(rg["len"]) == 0:
        return np.zeros((0, 2 if ss else 1, 3 + len(thresholds)), np.int64)
    return from_rows(rows_of(cells, rg, ss), thresholds)


def expected(cols_or_oracle, rg, signal, ss, thresholds, **params):
    return from_cells(de.cells(cols_or_oracle, rg, signal, ss, **params), rg, ss, thresholds)


def has_tie(rows):
    """does some range hold its (positive) maximum in more than one cell?"""
    return any(c.shape[1] and c[r].max() > 0 and np.count_nonzero(c[r] == c[r].max()) > 1 for c in rows for r in range(c.shape[0]))
