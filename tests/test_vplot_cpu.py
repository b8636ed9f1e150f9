"""CPU: the V-plot's expected side (tests/vplot_expected.py: one oracle bamProfile per row band) against a direct numpy
restatement and against its two marginals; the VPlot class from hand-made integers; the parameter rule at file level and
bamVPlot's own refusals, none of which needs a device."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import vplot_expected as ve

BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [60_000, 30_011]
GRID = (((0, 1000), 7), ((150, 300), 1), ((120, 5000), 64), ((0, 999), 1000))


@pytest.fixture(scope="module")
def small():
    """20,000 paired reads on two references, with a few lengths beyond the generator's own and tlens of either sign"""
    from bamsignals_amd.synth import synth_reads
    cols = synth_reads(20_000, REF_LEN, seed=17, paired=True, with_cigar=False)
    rng = np.random.default_rng(18)
    tl = cols["tlen"].astype(np.int64)
    far = rng.random(len(tl)) < 0.05
    tl[far] = rng.integers(0, 6000, int(far.sum())) * np.where(rng.random(int(far.sum())) < 0.5, -1, 1)
    cols["tlen"] = tl.astype(np.int32)
    return cols


def _ranges(w, seed):
    from bamsignals_amd.synth import synth_ranges
    rg = synth_ranges(40, w, REF_LEN, seed=seed)
    assert len(set(rg["strand"].tolist())) == 3
    return rg


@pytest.mark.parametrize("midpoint", [False, True])
@pytest.mark.parametrize("w", [1, 100, 2049])
def test_definition_is_the_numpy_restatement(small, w, midpoint):
    rg = _ranges(w, seed=w)
    total = 0
    for tf, lenbin in GRID:
        for binsize in sorted({1, 7, 50, w, w + 1}):
            for kw in (dict(), dict(mapqual=20, filteredF=1024)):
                want = ve.restated(small, rg, tf, lenbin, binsize, midpoint, **kw)
                got = ve.expected(small, rg, tf, lenbin, binsize, midpoint, **kw)
                assert got.dtype == np.int64 and got.shape == (tf[1] // lenbin + 1, -(-w // binsize))
                assert np.array_equal(got, want), (tf, lenbin, binsize, kw)
                total += int(got.sum())
    assert w < 2049 or total > 5000                      # (not vacuous)


@pytest.mark.parametrize("midpoint", [False, True])
def test_marginals(small, midpoint):
    rg = _ranges(2049, seed=2049)
    for tf, lenbin in GRID:
        for binsize in (1, 7, 2050):
            t = ve.restated(small, rg, tf, lenbin, binsize, midpoint)
            assert np.array_equal(t.sum(axis=1), ve.frag_marginal(small, rg, tf, lenbin, midpoint))
            assert np.array_equal(t.sum(axis=0), ve.profile_marginal(small, rg, tf, binsize, midpoint))
            assert t.sum() > 0


def test_a_minus_range_is_the_plus_range_mirrored(small):
    rg = _ranges(2049, seed=5)
    plus, minus = dict(rg, strand=np.ones_like(rg["strand"])), dict(rg, strand=-np.ones_like(rg["strand"]))
    for binsize in (1, 3):                                # 2049 = 3 * 683: whole bins mirror onto whole bins
        a = ve.expected(small, plus, (0, 1000), 7, binsize, True)
        b = ve.expected(small, minus, (0, 1000), 7, binsize, True)
        assert np.array_equal(a, b[:, ::-1]) and not np.array_equal(a, b)


def test_planted_fragments_have_a_known_answer():
    loc, w = 1000, 500
    for strand in (1, -1):
        rg = dict(rid=[0], loc=[loc], len=[w], strand=[strand])
        for length, reverse in ((147, False), (147, True), (200, False), (201, True)):
            cols = ve.merge_sorted([ve.planted(3, length, loc + 200, reverse=reverse)], 1)
            for midpoint in (False, True):
                rel = 200 + ((-1 if reverse else 1) * (length // 2) if midpoint else 0)
                rel = w - 1 - rel if strand < 0 else rel
                want = np.zeros((1000 // 7 + 1, -(-w // 50)), np.int64)
                want[length // 7, rel // 50] = 3
                assert np.array_equal(ve.expected(cols, rg, (0, 1000), 7, 50, midpoint), want), (strand, length, reverse, midpoint)


# ---- VPlot -----------------------------------------------------------------------------------------------------------
def test_vplot_object():
    from bamsignals_amd import FragSizes, VPlot
    c = np.arange(24, dtype=np.int64).reshape(4, 6)
    vp = VPlot(c, lenbin=10, binsize=25)
    assert vp.counts.dtype == np.int64 and vp.counts.shape == (4, 6) and vp.lenbin == 10 and vp.binsize == 25
    assert vp.lengths.tolist() == [0, 10, 20, 30] and vp.positions.tolist() == [0, 25, 50, 75, 100, 125]
    assert vp.n == int(c.sum())
    fs = vp.frag_sizes()
    assert isinstance(fs, FragSizes) and fs.lenbin == 10 and fs.counts.tolist() == c.sum(axis=1).tolist()
    assert vp.profile().tolist() == c.sum(axis=0).tolist() and vp.profile().dtype == np.int64
    assert vp.band(0, 39).tolist() == vp.profile().tolist()
    assert vp.band(10, 29).tolist() == (c[1] + c[2]).tolist()
    assert vp.band(30, 39).tolist() == c[3].tolist()
    for lo, hi in ((5, 19), (0, 18), (0, 20), (10, 9), (-10, 9), (0, 49), (20, 9)):
        with pytest.raises(ValueError):
            vp.band(lo, hi)
    assert repr(vp) == f"VPlot(rows=4, cols=6, lenbin=10, binsize=25, n={int(c.sum())})"
    with pytest.raises(ValueError):
        vp.counts[0, 0] = 1
    with pytest.raises(ValueError):
        vp.lengths[0] = 1
    with pytest.raises(ValueError):
        vp.positions[0] = 1
    for name in ("n", "lenbin", "binsize", "counts"):
        with pytest.raises(AttributeError):
            setattr(vp, name, 3)
    c[0, 0] = 99                                          # (the table is a copy)
    assert vp.counts[0, 0] == 0
    empty = VPlot(np.zeros((5, 0), np.int64), lenbin=2)
    assert empty.n == 0 and empty.profile().shape == (0,) and empty.frag_sizes().counts.tolist() == [0] * 5
    assert VPlot(np.full((2, 2), 2 ** 62, np.int64)).n == 2 ** 64          # exact past int64
    with pytest.raises(ValueError):
        VPlot(np.zeros(4, np.int64))


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    from bamsignals_amd import _lib, vplot
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    cap = re.search(r"#define\s+BSIG_VPLOT_MAX_CELLS\s+\(1 << (\d+)\)", txt)
    assert cap and 1 << int(cap.group(1)) == vplot.MAX_CELLS == _lib.VPLOT_MAX_CELLS == 2 ** 24
    assert vplot.MAX_ROWS == _lib.FRAG_MAX_ROWS == 16384
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4


def _call_vplot(len_bin=1, tlen_filter=(0, 1000), binsize=1, width=(100, 100)):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray(width, np.int32)
    codes, start, strand = np.arange(2, dtype=np.int32), np.full(2, 1000, np.int32), np.ones(2, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    out = np.zeros(8, np.int64)                           # (a refused call writes nothing)
    rc = lib.bsig_pileup_vplot(BAM.encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data,
                               strand.ctypes.data, tf.ctypes.data, len(tlen_filter), 0, binsize, 66, -1, 1, len_bin, 16385, -1,
                               out.ctypes.data)
    assert not out.any()
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


# the table test_vplot_gpu.py::test_errors runs through bsig_plan_create_vplot (with shift, ss, mode and threads, which only
# the plan call can express)
FILTER_MESSAGE = "the V-plot needs a 2-element tlen_filter"
PARAM_RULE = [
    (dict(tlen_filter=()), -1, FILTER_MESSAGE),
    (dict(tlen_filter=(50,)), -1, FILTER_MESSAGE),
    (dict(len_bin=0), -1, "len_bin must be greater or equal to 1"),
    (dict(binsize=0), -1, "provide a binsize greater or equal to 1"),
    (dict(binsize=-1), -1, "provide a binsize greater or equal to 1"),
    (dict(width=(100, 101)), -1, "all signals must have the same length"),
    (dict(tlen_filter=(0, 16384)), -1, "tlen_filter[1] / len_bin + 1 = 16385 rows, at most 16384 fit: choose a wider len_bin"),
    (dict(tlen_filter=(0, 163840), len_bin=10), -1,
     "tlen_filter[1] / len_bin + 1 = 16385 rows, at most 16384 fit: choose a wider len_bin"),
    (dict(tlen_filter=(0, 16383), width=(1025, 1025)), -1,
     "16384 rows x 1025 columns are more than 16777216 cells: choose a wider len_bin or binsize"),
    (dict(tlen_filter=(0, 9999), len_bin=10, binsize=2, width=(33556, 33556)), -1,
     "1000 rows x 16778 columns are more than 16777216 cells: choose a wider len_bin or binsize"),
]


@pytest.mark.parametrize("a,code,message", PARAM_RULE)
def test_parameter_rule_at_file_level(a, code, message):
    rc, msg, route = _call_vplot(**a)
    assert (rc, msg) == (code, message)
    assert route == b""                          # refused before the BAM is opened


# Which refusal wins, as tests/test_file_level_refusals_cpu.py pins it for the entry points that existed when its table was
# recorded (that table is not touched: the header declares bsig_pileup_vplot with its parameters on the lines after its
# name, which the table's enumeration of one-line declarations does not take).  The same faults, alone and in pairs: a the
# output missing, b a one-element tlen_filter, c a file that does not exist, d a chromosome the BAM lacks, e = b + c,
# f = b + d.  The V-plot judges its parameters before it opens the BAM, as the fragment-length histogram does.
REFUSALS = {
    "a": ({"output"}, (-1, "out is NULL")),
    "b": ({"filter"}, (-1, FILTER_MESSAGE)),
    "c": ({"file"}, (-2, "Fail to open BAM file <missing>")),
    "d": ({"chrom"}, (-4, "chromosome chrNone not present in the bam file")),
    "e": ({"filter", "file"}, (-1, FILTER_MESSAGE)),
    "f": ({"filter", "chrom"}, (-1, FILTER_MESSAGE)),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_which_refusal_wins_at_file_level(case):
    from bamsignals_amd import _lib
    lib = _lib.load()
    faults, want = REFUSALS[case]
    missing = os.path.join(GOLDEN, "no_such_file.bam")
    width, start, strand = np.full(2, 100, np.int32), np.full(2, 1000, np.int32), np.ones(2, np.int32)
    codes = np.arange(2, dtype=np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chrNone" if "chrom" in faults else b"chr2")
    tf = np.asarray((50,) if "filter" in faults else (0, 500), np.int32)
    out = np.zeros(4096, np.int64)
    rc = lib.bsig_pileup_vplot((missing if "file" in faults else BAM).encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data,
                               width.ctypes.data, strand.ctypes.data, tf.ctypes.data, len(tf), 0, 10, 66, -1, 1, 10, 16385, -1,
                               None if "output" in faults else out.ctypes.data)
    assert (rc, lib.bsig_last_error().decode().replace(missing, "<missing>")) == want
    assert lib.bsig_last_call_route() == b"" and not out.any()


def test_wrapper_refuses_before_any_native_call(monkeypatch):
    from bamsignals_amd import GRanges, bamVPlot, vplot, wrappers
    def boom(*a, **k):  # noqa: E306
        raise AssertionError("native call made")
    monkeypatch.setattr(wrappers, "pileup_vplot", boom)
    gr = GRanges(["chr1", "chr2"], [1, 50], width=[100, 100], strand=["+", "-"])
    no = "/nonexistent/file.bam"
    for bad in (0, -3, 2.5, "7", True, None):
        with pytest.raises(ValueError, match="lenbin"):
            bamVPlot(no, gr, lenbin=bad, verbose=False)
        with pytest.raises(ValueError, match="binsize"):
            bamVPlot(no, gr, binsize=bad, verbose=False)
    with pytest.raises(ValueError, match="all signals must have the same length"):
        bamVPlot(no, GRanges(["chr1", "chr2"], [1, 50], width=[100, 101], strand=["+", "-"]), verbose=False)
    with pytest.raises(ValueError, match=str(vplot.MAX_ROWS)):
        bamVPlot(no, gr, tlenFilter=(0, vplot.MAX_ROWS), verbose=False)
    wide = GRanges(["chr1"], [1], width=[1025], strand=["+"])
    with pytest.raises(ValueError, match="16384 rows x 1025 columns are more than 16777216 cells: choose a wider lenbin or binsize"):
        bamVPlot(no, wide, tlenFilter=(0, vplot.MAX_ROWS - 1), verbose=False)
    for tf in ((300, 100), (5,), (-1, 5)):
        with pytest.raises(ValueError, match="tlenFilter"):
            bamVPlot(no, gr, tlenFilter=tf, verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamVPlot(no, [("chr1", 1, 100)], verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamVPlot(no, gr, paired_end="ignore", verbose=False)
    with pytest.warns(UserWarning, match="not a multiple"), pytest.raises(AssertionError, match="native call made"):
        bamVPlot(no, gr, binsize=7, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for good in (dict(), dict(lenbin=2.0, binsize=50.0, paired_end="filter"), dict(tlenFilter=(0, vplot.MAX_ROWS - 1), binsize=100),
                     dict(tlenFilter=(0, 10 * vplot.MAX_ROWS - 1), lenbin=10, binsize=100)):
            with pytest.raises(AssertionError, match="native call made"):       # ... and a good call does get there
                bamVPlot(no, gr, verbose=False, **good)
