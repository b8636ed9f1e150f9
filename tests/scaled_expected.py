"""The expected side of the scaled-region tests (a helper, not a conftest): the definition, literally -- the C oracle's
per-base cells (tests/depthhist_expected.py: cells), split per range with the oracle's layout
(tests/summary_expected.py: rows_of), then np.add.at into bin c * N // w in 64-bit integers.  Never the GPU plan."""
import numpy as np

import depthhist_expected as de
from depthhist_expected import merge_sorted, oracle_reads, planted  # noqa: F401  (shared helpers)
from summary_expected import rows_of


def bin_of(w, N):
    """b(c) = floor(c * N / w) for c = 0 .. w - 1, int64"""
    return (np.arange(w, dtype=np.int64) * N) // w


def from_rows(rows, N):
    """(n, S, N) int64 from the per-range (S, w) cell arrays"""
    S = rows[0].shape[0] if rows else 1
    out = np.zeros((len(rows), S, N), np.int64)
    for i, c in enumerate(rows):
        w = c.shape[1]
        if w == 0:
            continue
        b = bin_of(w, N)
        for r in range(S):
            np.add.at(out[i, r], b, c[r])
    return out


def from_cells(cells, rg, ss, N):
    if len(rg["len"]) == 0:
        return np.zeros((0, 2 if ss else 1, N), np.int64)
    return from_rows(rows_of(cells, rg, ss), N)


def expected(cols_or_oracle, rg, signal, ss, N, **params):
    return from_cells(de.cells(cols_or_oracle, rg, signal, ss, **params), rg, ss, N)


def bin_sizes(w, N):
    """the cells of bin j: [ceil(j * w / N), ceil((j + 1) * w / N)), from the edges (Python integers: no width wraps)"""
    edges = [-((-j * int(w)) // int(N)) for j in range(int(N) + 1)]
    return np.asarray([b - a for a, b in zip(edges[:-1], edges[1:])], np.int64)
