"""CPU: the scaled regions' expected side (tests/scaled_expected.py: the oracle's cells added into bin c * N // w)
against what the definition implies -- N = 1 is the range's sum, N = w the cells, N | w the oracle's own binned signal --
and planted reads with a known answer; the bins' sizes; the header's constant; the argument errors that need no device;
ScaledSignals' methods from hand-made integers."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import depthhist_expected as de
import scaled_expected as sc
import summary_expected as se
from test_crosscorr_cpu import _small

BAM = os.path.join(GOLDEN, "randomBam.bam")
SIGNALS = [("coverage", False), ("ends", False), ("ends", True)]


def test_the_package_exports_the_feature():
    from bamsignals_amd import ScaledSignals, bamScaled  # noqa: F401
    import bamsignals_amd
    assert "bamScaled" in bamsignals_amd.__all__ and "ScaledSignals" in bamsignals_amd.__all__


def test_constants_are_the_headers():
    from bamsignals_amd import _lib, scaled
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    cap = int(re.search(r"#define\s+BSIG_SCALED_MAX_BINS\s+(\d+)", txt).group(1))
    assert cap == 2048 == _lib.SCALED_MAX_BINS == scaled.MAX_BINS
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4


# ---- the definition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signal,ss", SIGNALS)
def test_definition_at_its_corners(signal, ss):
    """N = 1: the range's sum; N = w: the cells; N = 2 w: cell c in bin 2 c; every N: the bins add up to the sum"""
    from oracle import oracle_c
    S = 2 if ss else 1
    some = 0
    for seed in (5, 6):
        cols, rg = _small(seed)
        orc = de.oracle_reads(cols)
        for mapqual in (0, 25):
            cells = de.cells(orc, rg, signal, ss, mapqual=mapqual)
            rows = se.rows_of(cells, rg, ss)
            sums = se.from_rows(rows, ())[..., 0]
            one = sc.from_cells(cells, rg, ss, 1)
            assert one.dtype == np.int64 and one.shape == (len(rows), S, 1) and np.array_equal(one[..., 0], sums)
            for N in (3, 7, 100, 2048):
                got = sc.from_cells(cells, rg, ss, N)
                assert got.shape == (len(rows), S, N) and np.array_equal(got.sum(axis=-1), sums), N
            for i, c in enumerate(rows):
                w = c.shape[1]
                one_rg = {k: np.asarray(v)[i:i + 1] for k, v in rg.items()}
                if w == 0:
                    assert not sc.from_rows([c], 5).any()
                    continue
                assert np.array_equal(sc.from_rows([c], w)[0], c)
                twice = sc.from_rows([c], 2 * w)[0]
                assert np.array_equal(twice[:, 0::2], c) and not twice[:, 1::2].any()
                # N | w: the oracle's own bins of w / N cells (a '-' range mirrored first, binned second, here as there)
                for N in (n for n in (1, 2, 3, 5, 7, 10, 50, 100) if w % n == 0):
                    got = sc.from_rows([c], N)[0]
                    if signal == "ends":
                        binned, _ = oracle_c.pileup_core(orc, one_rg, binsize=w // N, shift=0, ss=ss, mapqual=mapqual)
                        want = np.asarray(binned, np.int64).reshape(N, S).T
                    else:
                        # (the oracle has no binned coverage of its own: its per-base coverage, w / N cells a bin)
                        want = c.reshape(S, N, w // N).sum(axis=-1)
                    assert np.array_equal(got, want), (seed, i, N)
                    some += int(got.any())
    assert some > 20                                        # (not vacuous)


@pytest.mark.parametrize("N", [1, 3, 100, 2048])
@pytest.mark.parametrize("w", [1, 7, 99, 100, 101, 2047, 2049, 2_200_000])
def test_bin_sizes(w, N):
    from bamsignals_amd.scaled import bin_sizes
    size = sc.bin_sizes(w, N)
    assert size.shape == (N,) and int(size.sum()) == w
    assert set(size.tolist()) <= {w // N, -(-w // N)}
    assert np.array_equal(size, np.bincount(sc.bin_of(w, N), minlength=N))
    assert (w >= N) == bool((size > 0).all())
    assert np.array_equal(bin_sizes([w, 0], N), [size, np.zeros(N, np.int64)])      # (the package's own restatement)


def test_planted_reads_have_a_known_answer():
    loc, w = 1000, 500
    # forward reads of 40 bases: 5 beginning on cell 100 (of the '+' range), 3 on cell 200, 5 on cell 300
    cols = sc.merge_sorted([sc.planted(5, 0, loc + 100), sc.planted(5, 0, loc + 300), sc.planted(3, 0, loc + 200)], 1)
    plus = dict(rid=[0], loc=[loc], len=[w], strand=[1])
    minus = dict(rid=[0], loc=[loc], len=[w], strand=[-1])
    zero = [0] * 10
    # ten bins of 50 cells; on '-' cell c is the base loc + 499 - c
    assert sc.expected(cols, plus, "coverage", False, 10).tolist() == [[[0, 0, 200, 0, 120, 0, 200, 0, 0, 0]]]
    assert sc.expected(cols, minus, "coverage", False, 10).tolist() == [[[0, 0, 0, 200, 0, 120, 0, 200, 0, 0]]]
    assert sc.expected(cols, plus, "ends", False, 10).tolist() == [[[0, 0, 5, 0, 3, 0, 5, 0, 0, 0]]]
    assert sc.expected(cols, minus, "ends", False, 10).tolist() == [[[0, 0, 0, 5, 0, 3, 0, 5, 0, 0]]]
    # with strands: forward reads are sense on '+', antisense on '-'
    assert sc.expected(cols, plus, "ends", True, 10).tolist() == [[[0, 0, 5, 0, 3, 0, 5, 0, 0, 0], zero]]
    assert sc.expected(cols, minus, "ends", True, 10).tolist() == [[zero, [0, 0, 0, 5, 0, 3, 0, 5, 0, 0]]]
    # seven bins of 71 or 72 cells: bin 3 begins on cell ceil(1500 / 7) = 215, inside the middle pile (cells 200 .. 239);
    # mirrored, the pile is cells 260 .. 299 and bin 4 begins on cell ceil(2000 / 7) = 286
    assert sc.expected(cols, plus, "coverage", False, 7).tolist() == [[[0, 200, 45, 75, 200, 0, 0]]]
    assert sc.expected(cols, minus, "coverage", False, 7).tolist() == [[[0, 0, 200, 78, 42, 200, 0]]]
    assert sc.expected(cols, plus, "ends", True, 7).tolist() == [[[0, 5, 3, 0, 5, 0, 0], [0] * 7]]
    assert sc.expected(cols, minus, "ends", True, 7).tolist() == [[[0] * 7, [0, 0, 5, 0, 3, 5, 0]]]
    # a range without width, a range without reads, a range narrower than its bins, no ranges
    odd = dict(rid=[0, 0, 0, 0], loc=[loc, loc, 5000, loc + 138], len=[w, 0, 10, 3], strand=[1, 1, -1, 1])
    assert sc.expected(cols, odd, "coverage", False, 4).tolist() == [[[125, 195, 200, 0]], [[0] * 4], [[0] * 4], [[5, 5, 0, 0]]]
    assert sc.expected(cols, dict(rid=[], loc=[], len=[], strand=[]), "ends", True, 9).shape == (0, 2, 9)


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_before_any_native_call(monkeypatch):
    from bamsignals_amd import GRanges, bamScaled, wrappers
    def boom(*a, **k):  # noqa: E306
        raise AssertionError("native call made")
    monkeypatch.setattr(wrappers, "pileup_scaled", boom)
    monkeypatch.setattr(wrappers, "coverage_scaled", boom)
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    path = "/nonexistent/file.bam"
    for bad in (0, -1, 2049, 2.5, "7", True, None):
        with pytest.raises(ValueError, match="nbins"):
            bamScaled(path, gr, nbins=bad, verbose=False)
    with pytest.raises(ValueError, match="'signal' should be one of"):
        bamScaled(path, gr, signal="depth", verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamScaled(path, gr, signal="coverage", paired_end="midpoint", verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamScaled(path, gr, signal="ends", paired_end="extend", verbose=False)
    with pytest.raises(ValueError, match="ss must be FALSE"):
        bamScaled(path, gr, signal="coverage", ss=True, verbose=False)
    with pytest.raises(ValueError, match="ss must be TRUE or FALSE"):
        bamScaled(path, gr, signal="ends", ss=2, verbose=False)
    with pytest.raises(ValueError, match="tlenFilter"):
        bamScaled(path, gr, signal="ends", paired_end="filter", tlenFilter=(300, 100), verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamScaled(path, [("chr1", 1, 100)], verbose=False)
    for good in (dict(), dict(signal="ends"), dict(signal="ends", ss=True, paired_end="midpoint"), dict(nbins=1),
                 dict(signal="coverage", paired_end="extend", nbins=2048), dict(nbins=20.0), dict(nbins=np.int32(7))):
        with pytest.raises(AssertionError, match="native call made"):       # ... and a good call does get there
            bamScaled(path, gr, verbose=False, **good)


def _call_scaled(signal="coverage", n_bins=10, tlen_filter=(), ss=0, tspan=0, pe_mid=0):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray([100, 100], np.int32)
    codes, start, strand = np.arange(2, dtype=np.int32), np.full(2, 1000, np.int32), np.ones(2, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    out = np.zeros(2 * 2 * 2048, np.int64)
    head = (BAM.encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
            tf.ctypes.data, len(tlen_filter), 0)
    tail = (n_bins, 16385, -1, out.ctypes.data)
    if signal == "coverage":
        rc = lib.bsig_coverage_scaled(*head, 0, -1, tspan, *tail)
    else:
        rc = lib.bsig_pileup_scaled(*head, ss, 0, -1, pe_mid, *tail)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


# the table test_scaled_gpu.py::test_errors runs through bsig_plan_create_scaled (with what only the plan call can express)
PARAM_RULE = [
    (dict(signal="coverage", n_bins=0), -1, "n_bins must be between 1 and 2048"),
    (dict(signal="ends", ss=1, n_bins=0), -1, "n_bins must be between 1 and 2048"),
    (dict(signal="coverage", n_bins=2049), -1, "n_bins must be between 1 and 2048"),
    (dict(signal="ends", n_bins=2049), -1, "n_bins must be between 1 and 2048"),
    (dict(signal="ends", n_bins=-5), -1, "n_bins must be between 1 and 2048"),
    (dict(signal="ends", tlen_filter=(50,)), -1, "tlen_filter must have 0 or 2 elements"),
    (dict(signal="coverage", tspan=1), -1, "paired-end midpoint/extend needs a 2-element tlen_filter"),
    (dict(signal="ends", pe_mid=1), -1, "paired-end midpoint/extend needs a 2-element tlen_filter"),
]


@pytest.mark.parametrize("a,code,message", PARAM_RULE)
def test_parameter_rule_at_file_level(a, code, message):
    rc, msg, route = _call_scaled(**a)
    assert (rc, msg) == (code, message)
    assert route == b""                          # refused before the BAM is opened


# ---- ScaledSignals ---------------------------------------------------------------------------------------------------
def _hand_made():
    from bamsignals_amd import ScaledSignals
    # four ranges of widths 10, 2, 0 and 2^40 (sums past 32 bits) in four bins
    return ScaledSignals([[5, 0, 7, 9], [4, 0, 6, 0], [0, 0, 0, 0], [2 ** 41, 3 * 2 ** 38, 0, 2 ** 40]], [10, 2, 0, 2 ** 40], 4)


def test_read_only_object():
    from bamsignals_amd import ScaledSignals
    sg = _hand_made()
    assert len(sg) == 4 and sg.nbins == 4 and "n=4" in repr(sg) and "nbins=4" in repr(sg)
    for name in ("sums", "cells", "width"):
        a = getattr(sg, name)
        assert a.dtype == np.int64
        with pytest.raises(ValueError):
            a[0] = 1
        with pytest.raises(AttributeError):
            setattr(sg, name, a)
    with pytest.raises(AttributeError):
        sg.nbins = 5
    # 10 cells in four bins: edges 0, 3, 5, 8, 10; two cells in four: edges 0, 1, 1, 2, 2
    assert sg.cells.tolist() == [[3, 2, 3, 2], [1, 0, 1, 0], [0, 0, 0, 0], [2 ** 38] * 4]
    with pytest.raises(ValueError, match="sums"):
        ScaledSignals([[1, 2, 3]], [5], 4)
    with pytest.raises(ValueError, match="sums"):
        ScaledSignals([[[1, 2]], [[3, 4]]], [5, 5], 2)          # (n, 1, nbins): strands come as two rows
    with pytest.raises(ValueError, match="sums"):
        ScaledSignals([1, 2, 3], [5], 3)
    with pytest.raises(ValueError, match="width"):
        ScaledSignals([[1, 2]], [5, 6], 2)
    with pytest.raises(ValueError, match="width"):
        ScaledSignals([[1, 2]], [-5], 2)
    with pytest.raises(ValueError, match="nbins"):
        ScaledSignals([[1, 2]], [5], 0)


def test_mean_matrix_pooled():
    sg = _hand_made()
    num, den = sg.mean()
    assert np.array_equal(num, sg.sums) and np.array_equal(den, sg.cells)
    assert sg.mean(fractions=True).tolist() == [
        [Fraction(5, 3), Fraction(0), Fraction(7, 3), Fraction(9, 2)], [Fraction(4), None, Fraction(6), None], [None] * 4,
        [Fraction(8), Fraction(3), Fraction(0), Fraction(4)]]
    m = sg.matrix()
    assert m.dtype == np.float64 and m.shape == (4, 4)
    assert np.isnan(m).tolist() == [[False] * 4, [False, True, False, True], [True] * 4, [False] * 4]
    assert m[0].tolist() == [5 / 3, 0.0, 7 / 3, 4.5] and m[3].tolist() == [8.0, 3.0, 0.0, 4.0]
    s, c = sg.pooled()
    assert s.dtype == np.int64 and c.dtype == np.int64
    assert s.tolist() == [2 ** 41 + 9, 3 * 2 ** 38, 13, 2 ** 40 + 9] and c.tolist() == [2 ** 38 + 4, 2 ** 38 + 2, 2 ** 38 + 4, 2 ** 38 + 2]


def test_strand_split_shapes():
    from bamsignals_amd import ScaledSignals
    sg = ScaledSignals([[[4, 6], [0, 1]], [[1, 0], [2, 0]]], [10, 1], 2)
    assert sg.sums.shape == (2, 2, 2) and sg.cells.tolist() == [[5, 5], [1, 0]] and "rows=2" in repr(sg)
    assert sg.mean(fractions=True).tolist() == [[[Fraction(4, 5), Fraction(6, 5)], [Fraction(0), Fraction(1, 5)]],
                                                [[Fraction(1), None], [Fraction(2), None]]]
    assert sg.mean()[1].shape == (2, 2, 2)
    assert np.isnan(sg.matrix()).tolist() == [[[False, False]] * 2, [[False, True]] * 2]
    s, c = sg.pooled()
    assert s.tolist() == [[5, 6], [2, 1]] and c.tolist() == [6, 5]
