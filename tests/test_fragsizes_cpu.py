"""CPU: the fragment-length histogram's expected side (tests/fragsizes_expected.py: one oracle bamCount per row) against
a direct numpy restatement, planted fragments and the oracle's one bamCount; the argument errors that need no device;
FragSizes' methods from hand-made integers."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import fragsizes_expected as fe
from test_crosscorr_cpu import _small

BAM = os.path.join(GOLDEN, "randomBam.bam")


def _small_pairs(seed):
    """test_crosscorr_cpu's small seeded reads as paired ones: flags 99 / 147 / 83 / 163 (the strand bit kept), tlens of
    either sign up to 1,200, and a few duplicate-marked reads"""
    cols, rg = _small(seed)
    rng = np.random.default_rng(seed + 100)
    n = len(cols["pos"])
    neg = (cols["flag"] & 16) != 0
    first = rng.random(n) < 0.6
    flag = np.where(first, np.where(neg, 83, 99), np.where(neg, 147, 163))
    flag = np.where(rng.random(n) < 0.1, flag | 1024, flag)
    cols["flag"] = flag.astype(np.uint16)
    cols["tlen"] = (rng.integers(0, 1200, n) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.int32)
    return cols, rg


GRID = (((0, 1000), 7), ((150, 300), 1), ((0, 999), 1000), ((120, 5000), 64), ((0, 1000), 1))


@pytest.mark.parametrize("midpoint", [False, True])
def test_definition_is_the_numpy_restatement(midpoint):
    cols, rg = _small_pairs(5)
    total = 0
    for tf, lenbin in GRID:
        for kw in (dict(), dict(mapqual=20, filteredF=1024)):
            want = fe.restated(cols, rg, tf, lenbin, midpoint, **kw)
            got = fe.expected(cols, rg, tf, lenbin, midpoint, **kw)
            assert got.dtype == np.int64 and len(got) == tf[1] // lenbin + 1
            assert np.array_equal(got, want), (tf, lenbin, kw)
            total += int(got.sum())
    assert total > 500                                   # (not vacuous)


def test_planted_fragments_have_a_known_answer():
    loc, w = 1000, 500
    rg = dict(rid=[0], loc=[loc], len=[w], strand=[-1])
    for length, lenbin, k in ((147, 1, 5), (147, 10, 3), (1000, 7, 2), (0, 1, 4)):
        for reverse in (False, True):
            cols = fe.merge_sorted([fe.planted(k, length, loc + 200, reverse=reverse)], 1)
            for midpoint in (False, True):
                inside = not midpoint or (loc <= loc + 200 + (-1 if reverse else 1) * (length // 2) < loc + w)
                want = np.zeros(1000 // lenbin + 1, np.int64)
                want[length // lenbin] = k if inside else 0
                assert np.array_equal(fe.expected(cols, rg, (0, 1000), lenbin, midpoint), want), (length, lenbin, reverse, midpoint)
    # the 5' end inside, the midpoint outside: counts under "filter" only
    cols = fe.merge_sorted([fe.planted(3, 400, loc + w - 10)], 1)
    assert fe.expected(cols, rg, (0, 1000), 1, False)[400] == 3
    assert not fe.expected(cols, rg, (0, 1000), 1, True).any()
    # the second read of a pair and an improper pair never count
    other = fe.planted(3, 200, loc + 5)
    other["flag"] = np.asarray([163, 97, 65], np.int64)
    assert not fe.expected(fe.merge_sorted([other], 1), rg, (0, 1000), 1, False).any()


@pytest.mark.parametrize("midpoint", [False, True])
def test_rows_sum_to_one_count(midpoint):
    cols, rg = _small_pairs(6)
    for tf, lenbin in GRID:
        assert int(fe.expected(cols, rg, tf, lenbin, midpoint).sum()) == fe.whole_count(cols, rg, tf, midpoint) > 0


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_constant_is_the_headers():
    from bamsignals_amd import _lib, fragsizes
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    cap = int(re.search(r"#define\s+BSIG_FRAG_MAX_ROWS\s+(\d+)", txt).group(1))
    assert cap >= 16384 and fragsizes.MAX_ROWS == cap == _lib.FRAG_MAX_ROWS
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4


def test_wrapper_refuses_before_any_native_call(monkeypatch):
    from bamsignals_amd import GRanges, bamFragSizes, fragsizes, wrappers
    def boom(*a, **k):  # noqa: E306
        raise AssertionError("native call made")
    monkeypatch.setattr(wrappers, "pileup_frag", boom)
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    for bad in (0, -3, 2.5, "7", True, None):
        with pytest.raises(ValueError, match="lenbin"):
            bamFragSizes("/nonexistent/file.bam", gr, lenbin=bad, verbose=False)
    with pytest.raises(ValueError, match=str(fragsizes.MAX_ROWS)):
        bamFragSizes("/nonexistent/file.bam", gr, tlenFilter=(0, fragsizes.MAX_ROWS), verbose=False)
    with pytest.raises(ValueError, match=str(fragsizes.MAX_ROWS)):
        bamFragSizes("/nonexistent/file.bam", gr, tlenFilter=(0, 10 * fragsizes.MAX_ROWS), lenbin=10, verbose=False)
    with pytest.raises(ValueError, match="tlenFilter"):
        bamFragSizes("/nonexistent/file.bam", gr, tlenFilter=(300, 100), verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamFragSizes("/nonexistent/file.bam", [("chr1", 1, 100)], verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamFragSizes("/nonexistent/file.bam", gr, paired_end="ignore", verbose=False)
    for good in (dict(), dict(lenbin=2.0, paired_end="midpoint"), dict(tlenFilter=(0, fragsizes.MAX_ROWS - 1)),
                 dict(tlenFilter=(0, 10 * fragsizes.MAX_ROWS - 1), lenbin=10)):
        with pytest.raises(AssertionError, match="native call made"):       # ... and a good call does get there
            bamFragSizes("/nonexistent/file.bam", gr, verbose=False, **good)


def _call_frag(len_bin=1, tlen_filter=(0, 1000)):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray([100, 100], np.int32)
    codes, start, strand = np.arange(2, dtype=np.int32), np.full(2, 1000, np.int32), np.ones(2, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    out = np.zeros(_lib.FRAG_MAX_ROWS + 8, np.int64)
    rc = lib.bsig_pileup_frag(BAM.encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data,
                              strand.ctypes.data, tf.ctypes.data, len(tlen_filter), 0, 66, -1, 0, len_bin, 16385, -1,
                              out.ctypes.data)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


# the table test_fragsizes_gpu.py::test_errors runs through bsig_plan_create_frag (with shift, mode and threads, which only
# the plan call can express)
FILTER_MESSAGE = "the fragment-length histogram needs a 2-element tlen_filter"
PARAM_RULE = [
    (dict(tlen_filter=()), -1, FILTER_MESSAGE),
    (dict(tlen_filter=(50,)), -1, FILTER_MESSAGE),
    (dict(len_bin=0), -1, "len_bin must be greater or equal to 1"),
    (dict(tlen_filter=(0, 16384)), -1, "tlen_filter[1] / len_bin + 1 = 16385 rows, at most 16384 fit: choose a wider len_bin"),
    (dict(tlen_filter=(0, 163840), len_bin=10), -1,
     "tlen_filter[1] / len_bin + 1 = 16385 rows, at most 16384 fit: choose a wider len_bin"),
]


@pytest.mark.parametrize("a,code,message", PARAM_RULE)
def test_parameter_rule_at_file_level(a, code, message):
    rc, msg, route = _call_frag(**a)
    assert (rc, msg) == (code, message)
    assert route == b""                          # refused before the BAM is opened


# ---- FragSizes -------------------------------------------------------------------------------------------------------
def test_read_only_object():
    from bamsignals_amd import FragSizes
    fs = FragSizes([0, 3, 9, 4, 9, 2], lenbin=10)
    assert fs.counts.dtype == np.int64 and fs.lenbin == 10 and fs.n == 27
    assert fs.lengths.tolist() == [0, 10, 20, 30, 40, 50]
    with pytest.raises(ValueError):
        fs.counts[0] = 1
    with pytest.raises(ValueError):
        fs.lengths[0] = 1
    with pytest.raises(AttributeError):
        fs.n = 3
    with pytest.raises(AttributeError):
        fs.lenbin = 3


def test_mode_quantile_median_mean():
    from bamsignals_amd import FragSizes
    fs = FragSizes([0, 3, 9, 4, 9, 2])
    assert fs.mode() == 2                              # the first maximum on ties
    assert FragSizes([0, 3, 9, 4, 9, 2], lenbin=10).mode() == 20
    # cumulative 0 3 12 16 25 27
    assert fs.quantile(0) == 0                         # ceil(0) = 0 is reached by the first row
    assert fs.quantile(0.5) == 3 == fs.median()        # ceil(13.5) = 14: the first row with 14 or more is row 3 (16)
    assert fs.quantile(Fraction(12, 27)) == 2 and fs.quantile(Fraction(13, 27)) == 3
    assert fs.quantile(1) == 5
    assert FragSizes([0, 0, 5, 0], lenbin=7).quantile(1) == 14
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            fs.quantile(bad)
    assert fs.mean() == Fraction(3 * 1 + 9 * 2 + 4 * 3 + 9 * 4 + 2 * 5, 27)
    assert FragSizes([0, 3, 9, 4, 9, 2], lenbin=10).mean() == 10 * fs.mean()
    big = FragSizes([2 ** 62, 2 ** 62, 2 ** 62])      # sums past int64 stay exact
    assert big.n == 3 * 2 ** 62 and big.mean() == 1 and big.median() == 1


@pytest.mark.parametrize("lenbin", [1, 10])
def test_tlen_filter_on_a_ladder_with_known_tails(lenbin):
    from bamsignals_amd import FragSizes
    # 1,000 fragments: 2 + 3 in the low tail, 4 + 2 in the high one, the rest on three rungs
    c = np.zeros(60, np.int64)
    c[3], c[5], c[15], c[30], c[45], c[50], c[58] = 2, 3, 500, 300, 189, 4, 2
    fs = FragSizes(c, lenbin=lenbin)
    assert fs.n == 1000
    row = lambda lo, hi: (lo * lenbin, (hi + 1) * lenbin - 1)  # noqa: E731
    assert fs.tlen_filter(1) == row(3, 58)             # nothing may stay outside
    assert fs.tlen_filter(0.99) == row(15, 50)         # 5 a side: the low tail holds exactly 5, the high one 6: only its last 2 go
    assert fs.tlen_filter(0.995) == row(5, 50)         # 2 a side (2.5 rounded down)
    assert fs.tlen_filter(0.98) == row(15, 45)         # 10 a side: 4 + 2 go as well
    assert fs.tlen_filter(Fraction(1, 1000)) == row(15, 15)      # 499 a side: the median's row, never an empty interval
    lo, hi = fs.tlen_filter(0.99)
    inside = int(c[lo // lenbin:hi // lenbin + 1].sum())
    assert inside >= 990
    for bad in (0, 1.5, -1):
        with pytest.raises(ValueError):
            fs.tlen_filter(bad)


def test_empty_histogram_raises():
    from bamsignals_amd import FragSizes
    fs = FragSizes(np.zeros(11, np.int64), lenbin=3)
    assert fs.n == 0 and fs.lengths[-1] == 30
    for call in (fs.mode, fs.median, fs.mean, fs.tlen_filter, lambda: fs.quantile(0.5)):
        with pytest.raises(ValueError, match="n == 0"):
            call()
