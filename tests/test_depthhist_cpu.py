"""CPU: the depth histogram's expected side (tests/depthhist_expected.py: np.bincount of the oracle's cells) against a
direct numpy restatement and planted reads with a known answer; the header's constants; the argument errors that need no
device; DepthHist's methods from hand-made integers."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import depthhist_expected as de
from test_crosscorr_cpu import _small

BAM = os.path.join(GOLDEN, "randomBam.bam")


@pytest.mark.parametrize("signal,ss", [("coverage", False), ("ends", False), ("ends", True)])
def test_definition_is_the_numpy_restatement(signal, ss):
    total = 0
    for seed in (5, 6):
        cols, rg = _small(seed)
        for mapqual in (0, 25):
            want_cells = de.restated_cells(cols, rg, signal, ss, mapqual=mapqual)
            assert want_cells.size == de.n_cells(rg, ss)
            for V in (1, 2, 7, 100):
                got = de.expected(cols, rg, signal, ss, V, mapqual=mapqual)
                assert got.dtype == np.int64 and len(got) == V + 3
                want = np.concatenate([np.bincount(np.minimum(want_cells, V), minlength=V + 1), [want_cells.size, want_cells.sum()]])
                assert np.array_equal(got, want), (seed, mapqual, V)
                assert got[:V + 1].sum() == got[V + 1]
                total += int(got[V + 2])
    assert total > 2000                                  # (not vacuous)


def test_planted_reads_have_a_known_answer():
    loc, w = 1000, 500
    rg = dict(rid=[0], loc=[loc], len=[w], strand=[-1])
    # k forward reads of 40 bases starting on one base: 40 cells of coverage k; one 5'-end cell of value k
    for k in (1, 6, 7, 8):
        cols = de.merge_sorted([de.planted(k, 0, loc + 200)], 1)
        cov = de.expected(cols, rg, "coverage", False, 7)
        want = np.zeros(10, np.int64)
        want[0], want[min(k, 7)] = w - 40, 40
        want[8:] = [w, 40 * k]
        assert np.array_equal(cov, want), k
        for ss in (False, True):
            ends = de.expected(cols, rg, "ends", ss, 7)
            n = w * (2 if ss else 1)
            want = np.zeros(10, np.int64)
            want[0], want[min(k, 7)] = n - 1, 1
            want[8:] = [n, k]
            assert np.array_equal(ends, want), (k, ss)
    # a forward and a reverse read with their 5' ends on one base: one cell of 2 unstranded, two cells of 1 with strands
    cols = de.merge_sorted([de.planted(1, 0, loc + 9), de.planted(1, 0, loc + 9, reverse=True)], 1)
    assert de.expected(cols, rg, "ends", False, 3).tolist() == [w - 1, 0, 1, 0, w, 2]
    assert de.expected(cols, rg, "ends", True, 3).tolist() == [2 * w - 2, 2, 0, 0, 2 * w, 2]
    # a read that hangs over the range's end covers only the bases inside; a repeated range counts twice
    cols = de.merge_sorted([de.planted(2, 0, loc + w - 10)], 1)
    assert de.expected(cols, rg, "coverage", False, 3).tolist() == [w - 10, 0, 10, 0, w, 20]
    twice = dict(rid=[0, 0], loc=[loc, loc], len=[w, w], strand=[1, -1])
    assert de.expected(cols, twice, "coverage", False, 3).tolist() == [2 * (w - 10), 0, 20, 0, 2 * w, 40]
    # the sum moment is of the true values, not of the clipped ones
    assert de.expected(cols, rg, "coverage", False, 1).tolist() == [w - 10, 10, w, 20]


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    from bamsignals_amd import _lib, depthhist
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    cap = int(re.search(r"#define\s+BSIG_HIST_MAX_ROWS\s+(\d+)", txt).group(1))
    mom = int(re.search(r"#define\s+BSIG_HIST_MOMENTS\s+(\d+)", txt).group(1))
    assert cap == 8192 == _lib.HIST_MAX_ROWS and depthhist.MAX_DEPTH == cap - 1
    assert mom == 2 == _lib.HIST_MOMENTS
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4


def test_wrapper_refuses_before_any_native_call(monkeypatch):
    from bamsignals_amd import GRanges, bamDepthHist, depthhist, wrappers
    def boom(*a, **k):  # noqa: E306
        raise AssertionError("native call made")
    monkeypatch.setattr(wrappers, "pileup_hist", boom)
    monkeypatch.setattr(wrappers, "coverage_hist", boom)
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    path = "/nonexistent/file.bam"
    for bad in (0, -3, 2.5, "7", True, None, depthhist.MAX_DEPTH + 1):
        with pytest.raises(ValueError, match="maxdepth"):
            bamDepthHist(path, gr, maxdepth=bad, verbose=False)
    with pytest.raises(ValueError, match="'signal' should be one of"):
        bamDepthHist(path, gr, signal="depth", verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamDepthHist(path, gr, signal="coverage", paired_end="midpoint", verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamDepthHist(path, gr, signal="ends", paired_end="extend", verbose=False)
    with pytest.raises(ValueError, match="ss must be FALSE"):
        bamDepthHist(path, gr, signal="coverage", ss=True, verbose=False)
    with pytest.raises(ValueError, match="ss must be TRUE or FALSE"):
        bamDepthHist(path, gr, signal="ends", ss=2, verbose=False)
    with pytest.raises(ValueError, match="tlenFilter"):
        bamDepthHist(path, gr, signal="ends", paired_end="filter", tlenFilter=(300, 100), verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamDepthHist(path, [("chr1", 1, 100)], verbose=False)
    for good in (dict(), dict(signal="ends"), dict(signal="ends", ss=False, paired_end="midpoint"), dict(maxdepth=1),
                 dict(signal="coverage", paired_end="extend", maxdepth=depthhist.MAX_DEPTH), dict(maxdepth=20.0, ss=False)):
        with pytest.raises(AssertionError, match="native call made"):       # ... and a good call does get there
            bamDepthHist(path, gr, verbose=False, **good)


def _call_hist(signal="coverage", max_value=100, tlen_filter=(), ss=0, tspan=0, pe_mid=0):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray([100, 100], np.int32)
    codes, start, strand = np.arange(2, dtype=np.int32), np.full(2, 1000, np.int32), np.ones(2, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    out = np.zeros(_lib.HIST_MAX_ROWS + 8, np.int64)
    head = (BAM.encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
            tf.ctypes.data, len(tlen_filter), 0)
    if signal == "coverage":
        rc = lib.bsig_coverage_hist(*head, 0, -1, tspan, max_value, 16385, -1, out.ctypes.data)
    else:
        rc = lib.bsig_pileup_hist(*head, ss, 0, -1, pe_mid, max_value, 16385, -1, out.ctypes.data)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


# the table test_depthhist_gpu.py::test_errors runs through bsig_plan_create_hist (with what only the plan call can express)
RANGE_MESSAGE = "max_value must be between 1 and 8191"
PARAM_RULE = [
    (dict(signal="coverage", max_value=0), -1, RANGE_MESSAGE),
    (dict(signal="coverage", max_value=-5), -1, RANGE_MESSAGE),
    (dict(signal="coverage", max_value=8192), -1, RANGE_MESSAGE),
    (dict(signal="ends", max_value=0), -1, RANGE_MESSAGE),
    (dict(signal="ends", max_value=8192, ss=1), -1, RANGE_MESSAGE),
    (dict(signal="ends", max_value=1 << 30), -1, RANGE_MESSAGE),
    (dict(signal="ends", tlen_filter=(50,)), -1, "tlen_filter must have 0 or 2 elements"),
    (dict(signal="coverage", tspan=1), -1, "paired-end midpoint/extend needs a 2-element tlen_filter"),
    (dict(signal="ends", pe_mid=1), -1, "paired-end midpoint/extend needs a 2-element tlen_filter"),
]


@pytest.mark.parametrize("a,code,message", PARAM_RULE)
def test_parameter_rule_at_file_level(a, code, message):
    rc, msg, route = _call_hist(**a)
    assert (rc, msg) == (code, message)
    assert route == b""                          # refused before the BAM is opened


# ---- DepthHist -------------------------------------------------------------------------------------------------------
def test_read_only_object():
    from bamsignals_amd import DepthHist
    dh = DepthHist([10, 3, 0, 4, 2])
    assert dh.counts.dtype == np.int64 and dh.maxdepth == 4 and dh.n == 19 and dh.total == 3 + 12 + 8 and dh.saturated
    assert not DepthHist([10, 3, 0, 4, 0]).saturated
    with pytest.raises(ValueError):
        dh.counts[0] = 1
    for name in ("n", "total", "maxdepth", "counts", "saturated"):
        with pytest.raises(AttributeError):
            setattr(dh, name, 3)
    # the moments must fit the rows
    with pytest.raises(ValueError, match="add up"):
        DepthHist([10, 3, 0, 4, 2], n=20)
    with pytest.raises(ValueError, match="total"):
        DepthHist([10, 3, 0, 4, 2], total=22)             # two cells of at least 4 each
    with pytest.raises(ValueError, match="total"):
        DepthHist([10, 3, 0, 4, 0], total=16)             # nothing in the overflow row: the rows say 15


def test_mean_breadth_quantile():
    from bamsignals_amd import DepthHist
    dh = DepthHist([10, 3, 0, 4, 2], total=3 + 12 + 50 + 70)           # the overflow row's cells hold 50 and 70
    assert dh.saturated and dh.mean() == Fraction(135, 19)              # exact although saturated
    assert dh.breadth(0) == 1 and dh.breadth(1) == Fraction(9, 19) and dh.breadth(3) == Fraction(6, 19)
    assert dh.breadth(4) == Fraction(2, 19)
    for bad in (-1, 5, 2.0, True):
        with pytest.raises(ValueError):
            dh.breadth(bad)
    # cumulative 10 13 13 17 19
    assert dh.quantile(0) == 0 and dh.quantile(0.5) == 0 == dh.median()           # ceil(9.5) = 10 is reached by row 0
    assert dh.quantile(Fraction(11, 19)) == 1 and dh.quantile(Fraction(14, 19)) == 3
    assert dh.quantile(Fraction(18, 19)) == 4 == dh.quantile(1) == dh.maxdepth    # "at least 4"
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            dh.quantile(bad)
    assert dh.distinct() == 9
    assert dh.duplicate_fraction() == 1 - Fraction(9, 135)
    big = DepthHist([2 ** 62, 2 ** 62, 2 ** 62])          # sums past int64 stay exact
    assert big.n == 3 * 2 ** 62 and big.total == 3 * 2 ** 62 and big.mean() == 1 and big.median() == 1
    assert big.breadth(1) == Fraction(2, 3) and big.distinct() == 2 ** 63 and big.duplicate_fraction() == Fraction(1, 3)


def test_empty_histograms_raise():
    from bamsignals_amd import DepthHist
    dh = DepthHist(np.zeros(11, np.int64))
    assert dh.n == 0 and dh.total == 0 and dh.maxdepth == 10 and not dh.saturated
    for call in (dh.mean, dh.median, lambda: dh.breadth(1), lambda: dh.quantile(0.5)):
        with pytest.raises(ValueError, match="n == 0"):
            call()
    none = DepthHist([500, 0, 0])
    assert none.mean() == 0 and none.distinct() == 0
    for h in (dh, none):
        with pytest.raises(ValueError, match="total == 0"):
            h.duplicate_fraction()
