"""CPU: the per-range summaries' expected side (tests/summary_expected.py: sum / max / argmax / counts of the oracle's
cells) against a direct numpy restatement and planted reads with a known answer; the header's constants; the argument
errors that need no device; RangeSummary's methods from hand-made integers."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import summary_expected as se
from test_crosscorr_cpu import _small

BAM = os.path.join(GOLDEN, "randomBam.bam")


def test_the_package_exports_the_feature():
    from bamsignals_amd import RangeSummary, bamSummary  # noqa: F401
    import bamsignals_amd
    assert "bamSummary" in bamsignals_amd.__all__ and "RangeSummary" in bamsignals_amd.__all__


@pytest.mark.parametrize("signal,ss", [("coverage", False), ("ends", False), ("ends", True)])
def test_definition_is_the_numpy_restatement(signal, ss):
    thr = (1, 2, 3, 5)
    seen_max = 0
    for seed in (5, 6):
        cols, rg = _small(seed)
        for mapqual in (0, 25):
            got = se.expected(cols, rg, signal, ss, thr, mapqual=mapqual)
            assert got.dtype == np.int64 and got.shape == (len(rg["len"]), 2 if ss else 1, 3 + len(thr))
            # the restatement's cells: the ranges with width, one after the other, unmirrored; strands as two halves
            flat = se.restated_cells(cols, rg, signal, ss, mapqual=mapqual)
            at = 0
            for i, (w, strand) in enumerate(zip(rg["len"].tolist(), rg["strand"].tolist())):
                if w <= 0:
                    assert got[i, :, :3].tolist() == [[0, 0, -1]] * (2 if ss else 1) and not got[i, :, 3:].any()
                    continue
                n = w * (2 if ss else 1)
                c = flat[at:at + n].reshape(-1, w)
                at += n
                if strand < 0:                      # mirrored: the cells reversed, the strands swapped
                    c = c[::-1, ::-1]
                for r in range(c.shape[0]):
                    first = int(np.flatnonzero(c[r] == c[r].max())[0])
                    want = [int(c[r].sum()), int(c[r].max()), first] + [int((c[r] >= t).sum()) for t in thr]
                    assert got[i, r].tolist() == want, (seed, mapqual, i, r)
                    seen_max = max(seen_max, int(c[r].max()))
            assert at == len(flat)
    assert seen_max >= 3                                   # (not vacuous)


def test_planted_reads_have_a_known_answer():
    loc, w = 1000, 500
    # two piles of 5 forward reads of 40 bases, beginning on cells 100 and 300 (of the '+' range), and a lower one between
    cols = se.merge_sorted([se.planted(5, 0, loc + 100), se.planted(5, 0, loc + 300), se.planted(3, 0, loc + 200)], 1)
    thr = (1, 3, 4, 5, 6)
    plus = dict(rid=[0], loc=[loc], len=[w], strand=[1])
    minus = dict(rid=[0], loc=[loc], len=[w], strand=[-1])
    # coverage: 120 cells covered, 80 of them at 5; the LEFT pile's first cell on '+'
    assert se.expected(cols, plus, "coverage", False, thr).tolist() == [[[13 * 40, 5, 100, 120, 120, 80, 80, 0]]]
    # ... and on '-' the RIGHT pile, as a mirrored index: its last base loc + 339 is cell w - 1 - 339
    assert se.expected(cols, minus, "coverage", False, thr).tolist() == [[[13 * 40, 5, w - 1 - 339, 120, 120, 80, 80, 0]]]
    # 5' ends: three cells
    assert se.expected(cols, plus, "ends", False, thr).tolist() == [[[13, 5, 100, 3, 3, 2, 2, 0]]]
    assert se.expected(cols, minus, "ends", False, thr).tolist() == [[[13, 5, w - 1 - 300, 3, 3, 2, 2, 0]]]
    # with strands: forward reads are sense on '+', antisense on '-'; the empty row is (0, 0, 0)
    assert se.expected(cols, plus, "ends", True, thr).tolist() == [[[13, 5, 100, 3, 3, 2, 2, 0], [0] * 8]]
    assert se.expected(cols, minus, "ends", True, thr).tolist() == [[[0] * 8, [13, 5, w - 1 - 300, 3, 3, 2, 2, 0]]]
    # no thresholds, a range without width, a range without reads
    odd = dict(rid=[0, 0, 0], loc=[loc, loc, 5000], len=[w, 0, 10], strand=[1, 1, -1])
    assert se.expected(cols, odd, "coverage", False, ()).tolist() == [[[520, 5, 100]], [[0, 0, -1]], [[0, 0, 0]]]
    assert se.expected(cols, dict(rid=[], loc=[], len=[], strand=[]), "ends", True, (1,)).shape == (0, 2, 4)


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    from bamsignals_amd import _lib, summary
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    fixed = int(re.search(r"#define\s+BSIG_SUMMARY_FIXED\s+(\d+)", txt).group(1))
    cap = int(re.search(r"#define\s+BSIG_SUMMARY_MAX_THRESHOLDS\s+(\d+)", txt).group(1))
    assert fixed == 3 == _lib.SUMMARY_FIXED
    assert cap == 8 == _lib.SUMMARY_MAX_THRESHOLDS == summary.MAX_THRESHOLDS
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4


def test_wrapper_refuses_before_any_native_call(monkeypatch):
    from bamsignals_amd import GRanges, bamSummary, wrappers
    def boom(*a, **k):  # noqa: E306
        raise AssertionError("native call made")
    monkeypatch.setattr(wrappers, "pileup_summary", boom)
    monkeypatch.setattr(wrappers, "coverage_summary", boom)
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    path = "/nonexistent/file.bam"
    for bad in ((0,), (-3, 5), (2.5,), ("7",), (True,), (None,), 7, (5, 5), (10, 3), tuple(range(1, 10)), (2 ** 31,)):
        with pytest.raises(ValueError, match="thresholds"):
            bamSummary(path, gr, thresholds=bad, verbose=False)
    with pytest.raises(ValueError, match="'signal' should be one of"):
        bamSummary(path, gr, signal="depth", verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamSummary(path, gr, signal="coverage", paired_end="midpoint", verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamSummary(path, gr, signal="ends", paired_end="extend", verbose=False)
    with pytest.raises(ValueError, match="ss must be FALSE"):
        bamSummary(path, gr, signal="coverage", ss=True, verbose=False)
    with pytest.raises(ValueError, match="ss must be TRUE or FALSE"):
        bamSummary(path, gr, signal="ends", ss=2, verbose=False)
    with pytest.raises(ValueError, match="tlenFilter"):
        bamSummary(path, gr, signal="ends", paired_end="filter", tlenFilter=(300, 100), verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamSummary(path, [("chr1", 1, 100)], verbose=False)
    for good in (dict(), dict(signal="ends"), dict(signal="ends", ss=True, paired_end="midpoint"), dict(thresholds=()),
                 dict(signal="coverage", paired_end="extend", thresholds=tuple(range(1, 9))), dict(thresholds=[20.0, 2 ** 31 - 1])):
        with pytest.raises(AssertionError, match="native call made"):       # ... and a good call does get there
            bamSummary(path, gr, verbose=False, **good)


def _call_summary(signal="coverage", thresholds=(1, 10), tlen_filter=(), ss=0, tspan=0, pe_mid=0, null=False):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray([100, 100], np.int32)
    codes, start, strand = np.arange(2, dtype=np.int32), np.full(2, 1000, np.int32), np.ones(2, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    thr = np.asarray(list(thresholds) or [0], np.int32)
    out = np.zeros(2 * 2 * 16, np.int64)
    head = (BAM.encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
            tf.ctypes.data, len(tlen_filter), 0)
    tail = (len(thresholds), None if null else thr.ctypes.data, 16385, -1, out.ctypes.data)
    if signal == "coverage":
        rc = lib.bsig_coverage_summary(*head, 0, -1, tspan, *tail)
    else:
        rc = lib.bsig_pileup_summary(*head, ss, 0, -1, pe_mid, *tail)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


# the table test_summary_gpu.py::test_errors runs through bsig_plan_create_summary (with what only the plan call can express)
PARAM_RULE = [
    (dict(signal="coverage", thresholds=(0,)), -1, "thresholds must be at least 1 (0 given)"),
    (dict(signal="ends", thresholds=(3, -2)), -1, "thresholds must be at least 1 (-2 given)"),
    (dict(signal="coverage", thresholds=(5, 5)), -1, "thresholds must be strictly increasing"),
    (dict(signal="ends", ss=1, thresholds=(1, 9, 4)), -1, "thresholds must be strictly increasing"),
    (dict(signal="coverage", thresholds=tuple(range(1, 10))), -1, "n_thresholds must be between 0 and 8"),
    (dict(signal="ends", thresholds=(1, 2), null=True), -1, "thresholds is NULL"),
    (dict(signal="ends", tlen_filter=(50,)), -1, "tlen_filter must have 0 or 2 elements"),
    (dict(signal="coverage", tspan=1), -1, "paired-end midpoint/extend needs a 2-element tlen_filter"),
    (dict(signal="ends", pe_mid=1), -1, "paired-end midpoint/extend needs a 2-element tlen_filter"),
]


@pytest.mark.parametrize("a,code,message", PARAM_RULE)
def test_parameter_rule_at_file_level(a, code, message):
    rc, msg, route = _call_summary(**a)
    assert (rc, msg) == (code, message)
    assert route == b""                          # refused before the BAM is opened


# ---- RangeSummary ----------------------------------------------------------------------------------------------------
def _hand_made():
    from bamsignals_amd import RangeSummary
    # four ranges of widths 10, 4, 0, 2^40 (a sum past 32 bits); thresholds 1 and 20
    return RangeSummary(sum=[55, 0, 0, 2 ** 41], max=[30, 0, 0, 7], summit=[3, 0, -1, 2 ** 31 - 5],
                        covered=[[9, 2], [0, 0], [0, 0], [2 ** 39, 0]], width=[10, 4, 0, 2 ** 40], thresholds=(1, 20),
                        start=[101, 201, 301, 1], strand=["+", "-", "*", "-"])


def test_read_only_object():
    from bamsignals_amd import RangeSummary
    rs = _hand_made()
    assert len(rs) == 4 and rs.thresholds == (1, 20)
    for name in ("sum", "max", "summit", "covered", "width"):
        a = getattr(rs, name)
        assert a.dtype == np.int64
        with pytest.raises(ValueError):
            a[0] = 1
        with pytest.raises(AttributeError):
            setattr(rs, name, a)
    with pytest.raises(AttributeError):
        rs.thresholds = (2,)
    assert rs.covered.shape == (4, 2)
    with pytest.raises(ValueError, match="covered"):
        RangeSummary([1], [1], [0], [[1, 1]], [5], (1,))
    with pytest.raises(ValueError, match="thresholds"):
        RangeSummary([1], [1], [0], [[1, 1]], [5], (3, 2))
    with pytest.raises(ValueError, match="width"):
        RangeSummary([1], [1], [0], [[1]], [5, 6], (1,))


def test_mean_breadth_summit_failing():
    rs = _hand_made()
    num, den = rs.mean()
    assert num.tolist() == [55, 0, 0, 2 ** 41] and den.tolist() == [10, 4, 0, 2 ** 40]
    assert rs.mean(fractions=True).tolist() == [Fraction(11, 2), Fraction(0), None, Fraction(2)]
    num, den = rs.breadth(1)
    assert num.tolist() == [9, 0, 0, 2 ** 39] and den.tolist() == [10, 4, 0, 2 ** 40]
    assert rs.breadth(20, fractions=True).tolist() == [Fraction(1, 5), Fraction(0), None, Fraction(0)]
    for bad in (2, 0, 21, 1.0, True, "1"):
        with pytest.raises(ValueError, match="not one of the thresholds"):
            rs.breadth(bad)
    # '+': start + summit; '-': end - summit; no width: no position
    assert rs.summit_position().tolist() == [104, 204, 0, 2 ** 40 - (2 ** 31 - 5)]
    assert rs.failing(1, 0.9).tolist() == [1, 2, 3]              # 9/10 is not below 0.9
    assert rs.failing(1, Fraction(91, 100)).tolist() == [0, 1, 2, 3]
    assert rs.failing(1, 0.5).tolist() == [1, 2]                  # 2^39 / 2^40 is not below 1/2
    assert rs.failing(20, 0).tolist() == [2]                      # only the range without width
    with pytest.raises(ValueError):
        rs.failing(1, 1.5)
    with pytest.raises(ValueError):
        rs.failing(7, 0.5)


def test_strand_split_shapes():
    from bamsignals_amd import RangeSummary
    rs = RangeSummary(sum=[[4, 6], [0, 1]], max=[[2, 3], [0, 1]], summit=[[1, 9], [0, 4]],
                      covered=[[[3], [4]], [[0], [1]]], width=[10, 5], thresholds=(1,), start=[11, 21], strand=["+", "-"])
    assert rs.mean(fractions=True).tolist() == [[Fraction(2, 5), Fraction(3, 5)], [Fraction(0), Fraction(1, 5)]]
    assert rs.breadth(1)[0].tolist() == [[3, 4], [0, 1]] and rs.breadth(1)[1].tolist() == [[10, 10], [5, 5]]
    assert rs.summit_position().tolist() == [[12, 20], [25, 21]]
    assert rs.failing(1, 0.35).tolist() == [0, 1]                 # range 0 fails on its sense strand (3/10)
    assert rs.failing(1, 0.3).tolist() == [1]
    with pytest.raises(ValueError, match="does not know its ranges"):
        RangeSummary([1], [1], [0], [[1]], [5], (1,)).summit_position()
