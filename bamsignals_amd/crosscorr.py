"""bamCrossCorr: the strand cross-correlation over ranges -- the data's own value for ``shift``.

The reference's vignette asks the user to set ``shift`` to about half the average fragment length
(vignettes/bamsignals.Rmd:77-92).  For single-end data that length is read off the reads: a fragment of length L
sequenced from both ends puts a forward 5' end at p and a reverse 5' end at p + L - 1, so the lag at which the two
strands' 5' ends line up best is L - 1.  The sums are made on the GPU (bsig_pileup_xcorr); only ``maxlag + 6`` numbers
come back.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from . import wrappers as _w

# include/bamsignals_abi.h: BSIG_XCORR_MAX_LAG
MAX_LAG = _lib.XCORR_MAX_LAG


class CrossCorr:
    """The integers of a strand cross-correlation, read-only.

    ``cross[d]`` (int64, ``maxlag + 1``): the sum over all ranges and their cells x of sense[x] * antisense[x + d],
    nothing outside a range counted.  ``n_cells``: the sum of the ranges' widths.  ``sums`` / ``sumsqs``: (sense,
    antisense) sums of the per-base counts and of their squares over all cells."""

    __slots__ = ("_cross", "_n_cells", "_sums", "_sumsqs")

    def __init__(self, cross, n_cells, sums, sumsqs):
        c = np.array(cross, dtype=np.int64).reshape(-1)
        c.setflags(write=False)
        object.__setattr__(self, "_cross", c)
        object.__setattr__(self, "_n_cells", int(n_cells))
        object.__setattr__(self, "_sums", (int(sums[0]), int(sums[1])))
        object.__setattr__(self, "_sumsqs", (int(sumsqs[0]), int(sumsqs[1])))

    def __setattr__(self, name, value):
        raise AttributeError("CrossCorr is read-only")

    cross = property(lambda self: self._cross)
    n_cells = property(lambda self: self._n_cells)
    sums = property(lambda self: self._sums)
    sumsqs = property(lambda self: self._sumsqs)

    @property
    def maxlag(self):
        return len(self._cross) - 1

    def correlation(self):
        """Pearson correlation per lag, float64: ``(cross / N - mu_S mu_A) / (sigma_S sigma_A)`` with ``N = n_cells``,
        means and (population) standard deviations over all N cells.  The cells a lag loses at the ranges' ends are
        NOT taken out of N: lag d is normalised like lag 0, so values at different lags stay comparable as sums and
        the curve's maximum is ``cross``'s.  NaN at every lag where a variance is 0 (or there are no cells)."""
        n = self._n_cells
        out = np.full(len(self._cross), np.nan)
        if n <= 0:
            return out
        (s, a), (ss, aa) = self._sums, self._sumsqs
        # n^2 var = n sum(x^2) - sum(x)^2, in exact integers
        vs, va = n * ss - s * s, n * aa - a * a
        if vs <= 0 or va <= 0:
            return out
        den = float(np.sqrt(float(vs)) * np.sqrt(float(va)))
        num = self._cross.astype(object) * n - s * a          # n^2 cov, exact
        return np.asarray([float(x) for x in num], dtype=np.float64) / den

    def fragment_length(self, min_lag=0):
        """``argmax(cross[min_lag:]) + min_lag + 1``, the first maximum on ties: the fragment length whose two ends
        line up at the best lag.  ``min_lag`` steps over the read-length ("phantom") peak of short lags."""
        m = int(min_lag)
        if m != min_lag or m < 0 or m > self.maxlag:
            raise ValueError(f"min_lag must be a whole number between 0 and maxlag ({self.maxlag})")
        return int(np.argmax(self._cross[m:])) + m + 1

    def __repr__(self):
        return f"CrossCorr(maxlag={self.maxlag}, n_cells={self._n_cells}, sums={self._sums})"


def _maxlag(maxlag):
    if isinstance(maxlag, (bool, np.bool_)) or not isinstance(maxlag, (int, float, np.integer, np.floating)) \
            or not float(maxlag).is_integer():
        raise ValueError("maxlag must be a whole number of bases")
    m = int(maxlag)
    if m < 0 or m > MAX_LAG:
        raise ValueError(f"maxlag must be between 0 and {MAX_LAG}")
    return m


def bamCrossCorr(bampath, gr, maxlag=500, mapqual=0, paired_end=("ignore", "filter"), tlenFilter=None,  # noqa: N802,N803
                 filteredFlag=-1, verbose=True):
    """Strand cross-correlation of the 5' ends over the ranges ``gr``, lags ``0 .. maxlag`` (at most ``MAX_LAG``).

    With S, A the sense and antisense rows of ``bamProfile(bampath, gr[i], ss=True)`` (binsize 1, shift 0; a '-'
    range mirrored, '*' as '+'), ``cross[d] = sum_i sum_x S_i[x] * A_i[x + d]`` over the cells with x + d inside the
    range; ranges may differ in width, overlap or repeat.  ``mapqual``, ``paired_end`` ("ignore" or "filter"),
    ``tlenFilter`` and ``filteredFlag`` filter the reads as in ``bamProfile``.  Returns a ``CrossCorr``; a good value
    for the counting calls' ``shift`` is ``bamCrossCorr(...).fragment_length() // 2``."""
    if verbose:
        _w._print_sentence(bampath)
    m = _maxlag(maxlag)
    _w._check_gr(gr)
    pe = _w._match_arg(paired_end, ("ignore", "filter"), "paired.end")
    out = _w.pileup_xcorr(os.path.expanduser(str(bampath)), gr, _w.tlenFilter(tlenFilter, pe), mapqual, _w.flagMask(pe),
                          filteredFlag, m)
    return CrossCorr(out[:m + 1], out[m + 1], out[m + 2:m + 4], out[m + 4:m + 6])
