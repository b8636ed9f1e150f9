"""CPU: the strand cross-correlation's expected side (tests/crosscorr_expected.py) against a plain triple loop and against
planted pairs; the decomposition k_xcorr_tiles follows (bodies + antisense halos clipped at the range's end); the
argument errors that need no device; CrossCorr's two methods from hand-made integers."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import crosscorr_expected as xe

BAM = os.path.join(GOLDEN, "randomBam.bam")


def _small(seed, n=900, ref_len=(6000, 2500)):
    rng = np.random.default_rng(seed)
    rid = rng.integers(0, len(ref_len), n)
    pos = np.asarray([rng.integers(0, ref_len[r] - 60) for r in rid], np.int64)
    span = rng.integers(1, 60, n)
    cols = xe.merge_sorted([dict(rid=rid, pos=pos, end=pos + span - 1, flag=np.where(rng.random(n) < 0.5, 16, 0),
                                 mapq=rng.integers(0, 61, n))], len(ref_len))
    rg = dict(rid=np.asarray([0, 1, 0, 0, 1, 0, 0], np.int32), loc=np.asarray([100, 0, 100, 5800, -20, 3000, 40], np.int32),
              len=np.asarray([700, 2500, 700, 400, 90, 0, 3], np.int32), strand=np.asarray([1, -1, 1, 0, 1, -1, -1], np.int32))
    return cols, rg


def test_helper_is_the_triple_loop():
    from oracle import oracle_c
    cols, rg = _small(1)
    maxlag = 120
    out, off = oracle_c.pileup_core(xe.oracle_reads(cols), rg, binsize=1, shift=0, ss=True, mapqual=7)
    cross, mom = [0] * (maxlag + 1), [0] * 5
    for i in range(len(rg["len"])):
        s, a = (v.tolist() for v in xe.rows(out, off, i))
        w = len(s)
        mom[0] += w
        for x in range(w):
            mom[1] += s[x]; mom[2] += a[x]; mom[3] += s[x] * s[x]; mom[4] += a[x] * a[x]
        for d in range(maxlag + 1):
            for x in range(0, w - d):
                cross[d] += s[x] * a[x + d]
    got_c, got_m = xe.expected(cols, rg, maxlag, mapqual=7)
    assert got_c.tolist() == cross and got_m.tolist() == mom
    assert sum(cross) > 0 and mom[0] == int(np.sum(rg["len"]))


def test_planted_pairs_have_a_known_answer():
    """k pairs d apart and nothing else: cross is k at lag d and 0 elsewhere, on either strand -- mirroring a range
    swaps the strands' roles AND the order of a pair's ends, so the reverse 5' end stays d cells behind its partner"""
    p = np.asarray([1000, 1300, 1700, 2100, 2350], np.int64)
    for d in (0, 1, 37, 200):
        fwd = dict(rid=np.zeros(5, np.int64), pos=p, end=p + 29, flag=np.zeros(5, np.int64))
        rev = dict(rid=np.zeros(5, np.int64), pos=p + d - 29, end=p + d, flag=np.full(5, 16, np.int64))
        cols = xe.merge_sorted([fwd, rev], 1)
        for strand in (1, 0, -1):
            cross, mom = xe.expected(cols, dict(rid=[0], loc=[900], len=[1700], strand=[strand]), 200)
            want = np.zeros(201, np.int64)
            want[d] = 5
            assert np.array_equal(cross, want), (d, strand)
            assert mom.tolist() == [1700, 5, 5, 5, 5]
    # a pair whose reverse end lies beyond the range's last base does not count
    cross, mom = xe.expected(cols, dict(rid=[0], loc=[900], len=[2350 + 200 - 900], strand=[1]), 200)
    assert cross[200] == 4 and mom.tolist() == [1650, 5, 4, 5, 4]


@pytest.mark.parametrize("body", [16, 50, 64, 333, 5000])
def test_bodies_and_halos_sum_to_the_definition(body):
    """what a workgroup adds for a tile: S over the body x A over body + halo, the halo min(maxlag, cells left)"""
    from oracle import oracle_c
    cols, rg = _small(2)
    maxlag = 150                                  # (bodies of 16 .. 64: a halo spans several bodies)
    out, off = oracle_c.pileup_core(xe.oracle_reads(cols), rg, binsize=1, shift=0, ss=True)
    cross = np.zeros(maxlag + 1, np.int64)
    for i in range(len(rg["len"])):
        s, a = xe.rows(out, off, i)
        w = len(s)
        for c0 in range(0, w, body):
            nb = min(body, w - c0)
            halo = min(maxlag, w - c0 - nb)
            img = np.zeros(body + maxlag, np.int64)          # cells behind the tile's nc stay zero
            img[:nb + halo] = a[c0:c0 + nb + halo]
            for x in range(nb):
                if s[c0 + x]:
                    cross += s[c0 + x] * img[x:x + maxlag + 1]
    assert np.array_equal(cross, xe.expected(cols, rg, maxlag)[0])


def test_c_route_is_numpy_route():
    cols, rg = _small(3)
    for kw in (dict(), dict(mapqual=20, filteredF=16)):
        c, n = xe.expected(cols, rg, 80, route="c", **kw), xe.expected(cols, rg, 80, route="np", **kw)
        assert np.array_equal(c[0], n[0]) and np.array_equal(c[1], n[1])


def test_register_flush_bound():
    """k_xcorr_tiles' 32-bit register per lag and tile: sum(S) + sum(A) <= 2^15 reads bound a lag's sum by 2^28"""
    n = 32_768
    assert max(s * (n - s) for s in (n // 2 - 1, n // 2, n // 2 + 1)) == 2 ** 28 < 2 ** 32


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_constant_is_the_headers():
    from bamsignals_amd import _lib, crosscorr
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    cap = int(re.search(r"#define\s+BSIG_XCORR_MAX_LAG\s+(\d+)", txt).group(1))
    assert cap >= 2047 and crosscorr.MAX_LAG == cap == _lib.XCORR_MAX_LAG
    assert int(re.search(r"#define\s+BSIG_XCORR_MOMENTS\s+(\d+)", txt).group(1)) == _lib.XCORR_MOMENTS == 5
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4


def test_wrapper_refuses_before_any_device_call(monkeypatch):
    from bamsignals_amd import GRanges, bamCrossCorr, crosscorr, wrappers
    def boom(*a, **k):  # noqa: E306
        raise AssertionError("native call made")
    monkeypatch.setattr(wrappers, "pileup_xcorr", boom)
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    for bad in (-1, crosscorr.MAX_LAG + 1, 2.5, "7", True):
        with pytest.raises(ValueError, match="maxlag"):
            bamCrossCorr("/nonexistent/file.bam", gr, maxlag=bad, verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamCrossCorr("/nonexistent/file.bam", [("chr1", 1, 100)], verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamCrossCorr("/nonexistent/file.bam", gr, paired_end="midpoint", verbose=False)
    with pytest.raises(AssertionError, match="native call made"):       # ... and a good call does get there
        bamCrossCorr("/nonexistent/file.bam", gr, maxlag=2.0, paired_end="filter", verbose=False)


def _call_xcorr(max_lag=10, tlen_filter=()):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray([100, 100], np.int32)
    codes, start, strand = np.arange(2, dtype=np.int32), np.full(2, 1000, np.int32), np.ones(2, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    out = np.zeros(4096, np.int64)
    rc = lib.bsig_pileup_xcorr(BAM.encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data,
                               strand.ctypes.data, tf.ctypes.data, len(tlen_filter), 0, 0, -1, max_lag, 16385, -1,
                               out.ctypes.data)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


# the table test_crosscorr_gpu.py::test_errors runs through bsig_plan_create_xcorr (with shift, pe_mid and binsize, which
# only the plan call can express)
LAG_MESSAGE = "max_lag must be between 0 and 2047"
PARAM_RULE = [
    (dict(max_lag=-1), -1, LAG_MESSAGE),
    (dict(max_lag=2048), -1, LAG_MESSAGE),
    (dict(tlen_filter=(50,)), -1, "tlen_filter must have 0 or 2 elements"),
]


@pytest.mark.parametrize("a,code,message", PARAM_RULE)
def test_parameter_rule_at_file_level(a, code, message):
    rc, msg, route = _call_xcorr(**a)
    assert (rc, msg) == (code, message)
    assert route == b""                          # refused before the decode


# ---- CrossCorr -------------------------------------------------------------------------------------------------------
def test_read_only_object_and_fragment_length():
    from bamsignals_amd import CrossCorr
    cc = CrossCorr([3, 9, 4, 9, 2], 50, (6, 7), (10, 13))
    assert cc.cross.dtype == np.int64 and cc.maxlag == 4 and cc.n_cells == 50 and cc.sums == (6, 7) and cc.sumsqs == (10, 13)
    with pytest.raises(ValueError):
        cc.cross[0] = 1
    with pytest.raises(AttributeError):
        cc.n_cells = 3
    assert cc.fragment_length() == 2                 # first maximum on ties: lag 1 -> length 2
    assert cc.fragment_length(min_lag=2) == 4
    assert cc.fragment_length(min_lag=4) == 5
    for bad in (-1, 5, 1.5):
        with pytest.raises(ValueError):
            cc.fragment_length(min_lag=bad)


def test_correlation_is_the_formula_in_exact_rationals():
    cols, rg = _small(4, n=2500)
    cross, mom = xe.expected(cols, rg, 100)
    from bamsignals_amd import CrossCorr
    cc = CrossCorr(cross, mom[0], mom[1:3], mom[3:5])
    n, s, a, ss, aa = (int(v) for v in mom)
    vs, va = Fraction(ss, n) - Fraction(s, n) ** 2, Fraction(aa, n) - Fraction(a, n) ** 2
    assert vs > 0 and va > 0
    got = cc.correlation()
    assert got.dtype == np.float64 and got.shape == (101,)
    # the square root of an exact rational, to 60 digits: far more than a double holds
    scale = 10 ** 60
    sd = Fraction(math.isqrt(int(vs * va * scale * scale)), scale)
    worst = Fraction(0)
    for d in range(101):
        want = (Fraction(int(cross[d]), n) - Fraction(s, n) * Fraction(a, n)) / sd
        worst = max(worst, abs(Fraction(float(got[d])) - want))
    assert worst < Fraction(1, 10 ** 9)
    # ... and the bound tells right from wrong here: one count more or less in cross moves the value by 1 / (N sd)
    step = 1 / (n * sd)
    assert step > Fraction(1, 10 ** 6)
    assert float(worst) < 1e-12                      # float64 rounding of this formula: orders below the bound


def test_correlation_nan_where_a_variance_is_zero():
    from bamsignals_amd import CrossCorr
    assert np.all(np.isnan(CrossCorr([0, 0], 10, (0, 4), (0, 6)).correlation()))         # no sense read
    assert np.all(np.isnan(CrossCorr([40, 40], 10, (10, 20), (10, 40)).correlation()))   # both constant
    assert np.all(np.isnan(CrossCorr([0], 0, (0, 0), (0, 0)).correlation()))             # no cells
    c = CrossCorr([2, 0], 4, (2, 2), (2, 2)).correlation()          # S = A = [1, 1, 0, 0]: r(0) = 1
    assert c[0] == 1.0 and c[1] == -1.0
