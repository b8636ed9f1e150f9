"""CPU: keepDup.  The keyword and its argument errors, which need no device and no library; the header against _lib; the
new symbols; the file-level refusals of the two new entry points against a table written here; the expected side
(tests/capped_expected.py) against what the definition implies and against planted piles with hand-computed answers; and
the capped plans' arithmetic (planmath.h) through its stand-alone sanitizer driver against a restatement in Python."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import capped_expected as ce
import resized_expected as rz
from test_crosscorr_cpu import _small

BAM = os.path.join(GOLDEN, "randomBam.bam")
MISSING = os.path.join(GOLDEN, "no_such_file.bam")
HUGE = 2 ** 31 - 1


# ---- the keyword -----------------------------------------------------------------------------------------------------
def test_three_functions_take_the_keyword_and_no_other():
    import bamsignals_amd as ba
    for fn in (ba.bamCount, ba.bamProfile, ba.bamCoverage):
        p = inspect.signature(fn).parameters["keepDup"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__
        assert "keepDup" in fn.__doc__ and "min(e_s[p], k)" in fn.__doc__
    for name in ("bamCrossCorr", "bamFragSizes", "bamDepthHist", "bamSummary", "bamScaled"):
        assert "keepDup" not in inspect.signature(getattr(ba, name)).parameters, name


@pytest.fixture
def no_library(monkeypatch):
    """any touch of the library fails the test"""
    from bamsignals_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _gr():
    from bamsignals_amd import GRanges
    return GRanges(["chr1"], [100], [50], ["+"])


def test_argument_errors_come_before_the_library(no_library):
    import bamsignals_amd as ba
    gr = _gr()
    calls = {
        "count": lambda **kw: ba.bamCount("x.bam", gr, verbose=False, **kw),
        "profile": lambda **kw: ba.bamProfile("x.bam", gr, verbose=False, **kw),
        "coverage": lambda **kw: ba.bamCoverage("x.bam", gr, verbose=False, fragLength=100, **kw),
    }
    for name, call in calls.items():
        for bad, words in ((0, "at least 1"), (-3, "at least 1"), (2 ** 31, "at most 2147483647"), (1.5, "whole number"),
                           (True, "whole number"), ("2", "whole number")):
            with pytest.raises(ValueError, match=words):
                call(keepDup=bad)
        other = "extend" if name == "coverage" else "midpoint"
        with pytest.raises(ValueError, match="paired-end duplicate is a fragment with both ends equal"):
            call(keepDup=1, paired_end=other)
        if name != "count":
            for kw in (dict(aggregate=True), dict(runs=True)):
                with pytest.raises(ValueError, match="out of scope"):
                    call(keepDup=1, **kw)
    with pytest.raises(ValueError, match="paired-end duplicate"):
        ba.bamProfile("x.bam", gr, verbose=False, keepDup=2, paired_end="filter")
    with pytest.raises(ValueError, match="duplicates of different lengths have no defined survivor"):
        ba.bamCoverage("x.bam", gr, verbose=False, keepDup=1)
    # a whole float is a whole number, as for fragLength -- it reaches the library (and this fixture says so)
    with pytest.raises(AssertionError, match="the library was touched"):
        ba.bamCount("x.bam", gr, verbose=False, keepDup=2.0)


def test_constants_are_the_headers():
    from bamsignals_amd import _lib, wrappers
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4
    assert eval(re.search(r"#define\s+BSIG_FRAG_LEN_MAX\s+\((.+)\)", txt).group(1)) == wrappers.MAX_FRAG_LENGTH
    assert _lib.KEEP_DUP_MAX == 2 ** 31 - 1 == np.iinfo(np.int32).max
    # the two file-level calls stand with their parameters below their names (the recorded table of refusals lists the others)
    for name in ("bsig_pileup_capped", "bsig_coverage_capped"):
        assert re.search(r"^int %s\(\n    const char \*bampath" % name, txt, re.M), name


def test_new_symbols_are_exported():
    from bamsignals_amd import _lib, device, wrappers
    lib = _lib.load()
    for name in ("bsig_plan_create_capped", "bsig_plan_capped_cells", "bsig_plan_capped_runs", "bsig_plan_run_capped",
                 "bsig_plan_run_capped_host", "bsig_pileup_capped", "bsig_coverage_capped"):
        assert hasattr(lib, name), name
    assert lib.bsig_abi_version() == 4
    assert lib.bsig_plan_capped_cells(None) == 0 and lib.bsig_plan_capped_runs(None) == 0
    assert hasattr(device, "CappedPlan") and hasattr(wrappers, "pileup_capped") and hasattr(wrappers, "coverage_capped")


# ---- file-level refusals (the form of tests/test_file_level_refusals_cpu.py, which stays as recorded) ---------------------
PILEUP = dict(mapqual=0, binsize=1, shift=0, ss=0, requiredF=0, filteredF=-1, pe_mid=0, keep_dup=1, maxgap=16385, device=-1)
COVER = dict(mapqual=0, requiredF=0, filteredF=-1, tspan=0, frag_len=150, keep_dup=1, maxgap=16385, device=-1, binsize=1, ss=0)
ENTRIES = {"bsig_pileup_capped": PILEUP, "bsig_coverage_capped": COVER}
FAULTS = {"a": {"output"}, "b": {"filter"}, "c": {"file"}, "d": {"chrom"}, "e": {"filter", "file"}, "f": {"filter", "chrom"},
          "off": {"offsets"}}
OWN = {"bsig_pileup_capped": {"g:keep": dict(keep_dup=0), "g:mid": dict(pe_mid=1), "g:bins": dict(binsize=0, keep_dup=-1)},
       "bsig_coverage_capped": {"g:keep": dict(keep_dup=0), "g:span": dict(tspan=1), "g:length": dict(frag_len=0),
                                "g:long": dict(frag_len=(1 << 24) + 1), "g:bins": dict(binsize=65537)}}
NO_FILE = (-2, "Fail to open BAM file <missing>")
NO_CHROM = (-4, "chromosome chrNone not present in the bam file")
NO_RULE = (-1, "keep_dup caps single-end reads: it takes no template-length rule (n_tlen_filter must be 0)")
PAIRED = "a paired-end duplicate is a fragment with both ends equal, which a 5' end and a strand do not identify: %s must be 0 with keep_dup"
EXPECTED = {
    "bsig_pileup_capped": {
        "a": (-1, "out is NULL"), "b": NO_RULE, "c": NO_FILE, "d": NO_CHROM, "e": NO_RULE, "f": NO_RULE, "off": (-1, "offsets missing"),
        "g:keep": (-1, "keep_dup must be at least 1 (0 given)"), "g:mid": (-1, PAIRED % "pe_mid"),
        "g:bins": (-1, "keep_dup must be at least 1 (-1 given)")},
    "bsig_coverage_capped": {
        "a": (-1, "out is NULL"), "b": NO_RULE, "c": NO_FILE, "d": NO_CHROM, "e": NO_RULE, "f": NO_RULE, "off": (-1, "offsets missing"),
        "g:keep": (-1, "keep_dup must be at least 1 (0 given)"), "g:span": (-1, PAIRED % "tspan"),
        "g:length": (-1, "duplicates of different lengths have no defined survivor: bamCoverage takes keep_dup with a fragment length only"),
        "g:long": (-1, "the fragment length must be between 1 and 16777216 (16777217 given)"),
        "g:bins": (-1, "coverage bins are at most 65536 bases wide (bamProfile / bamCount count at that scale)")},
}


def _call(name, case):
    """one call on two ranges of width 100 with the case's faults (a case of the call's own comes with a missing file, so
    that it is seen to win before any I/O); (code, message, route)"""
    from bamsignals_amd import _lib
    lib = _lib.load()
    faults = FAULTS[case] if case in FAULTS else {"file"}
    mid = dict(ENTRIES[name], **OWN[name].get(case, {}))
    n = 2
    width, start, strand = np.full(n, 100, np.int32), np.full(n, 1000, np.int32), np.ones(n, np.int32)
    codes = np.arange(n, dtype=np.int32) % 2
    levels = (C.c_char_p * 2)(b"chr1", b"chrNone" if "chrom" in faults else b"chr2")
    tf = np.asarray((50,) if "filter" in faults else (0,), np.int32)
    path = MISSING if "file" in faults else BAM
    head = (path.encode(), n, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
            tf.ctypes.data, 1 if "filter" in faults else 0)
    out, off = np.zeros(4096, np.int32), np.zeros(n + 1, np.int64)
    lib.bsig_layout(n, width.ctypes.data, mid["binsize"], mid["ss"], off.ctypes.data)
    tail = (None if "output" in faults else out.ctypes.data, None if faults & {"output", "offsets"} else off.ctypes.data)
    rc = getattr(lib, name)(*head, *mid.values(), *tail)
    return rc, lib.bsig_last_error().decode().replace(MISSING, "<missing>"), lib.bsig_last_call_route()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_file_level_refusals(name):
    assert set(EXPECTED[name]) == set(FAULTS) | set(OWN[name])
    for case, want in EXPECTED[name].items():
        code, message, route = _call(name, case)
        assert (code, message) == want, (name, case)
        assert route == b"", (name, case)


# ---- the expected side against what the definition implies ---------------------------------------------------------------
def _rows(flat, off, i, ss):
    v = flat[off[i]:off[i + 1]]
    return v.reshape(-1, 2).T if ss else v


@pytest.mark.parametrize("ss", [False, True])
def test_ends_at_the_definitions_corners(ss):
    from oracle import oracle_c
    seen_capped = 0
    for seed in (5, 6):
        cols, rg = _small(seed)
        # piles, so that a cap of 1 or 2 bites
        cols = ce.merge_sorted([cols_part(cols), ce.planted(7, 0, 300), ce.planted(4, 0, 420, reverse=True),
                                ce.planted(3, 0, 5900, rid=0)], 2)
        orc = ce.oracle_reads(cols)
        for shift in (0, 13, -40):
            cells = ce.stranded_cells(orc, rg, shift=shift, mapqual=3)
            top = max(int(c.max(initial=0)) for c in cells)
            assert top >= 7
            for binsize in (1, 7, 200, 10_000, -1):
                plain, off = oracle_c.pileup_core(orc, rg, binsize=binsize, shift=shift, ss=ss, mapqual=3)
                # k at or above the largest cell: the oracle's own uncapped signal, binned and stranded
                for k in (top, HUGE):
                    got, goff = ce.ends(orc, rg, k, binsize, ss, shift=shift, mapqual=3)
                    assert np.array_equal(goff, off) and np.array_equal(got, plain), (seed, shift, binsize, k)
                # every binned result is the reduceat of the per-base one
                for k in (1, 2, 5):
                    base, boff = ce.ends(orc, rg, k, 1, True, shift=shift, mapqual=3)
                    got, goff = ce.ends(orc, rg, k, binsize, ss, shift=shift, mapqual=3)
                    assert np.array_equal(goff, off)
                    for i in range(len(rg["len"])):
                        b = _rows(base, boff, i, True)
                        w = b.shape[1]
                        edges = np.arange(0, w, binsize) if binsize > 0 else np.zeros(1, np.int64)
                        want = np.add.reduceat(b, edges, axis=1) if w else np.zeros((2, 1 if binsize <= 0 else 0), np.int64)
                        want = want if ss else want.sum(axis=0)
                        assert np.array_equal(_rows(got, goff, i, ss), want), (seed, shift, binsize, k, i)
                    seen_capped += int(got.sum() < plain.sum())
            # k = 1, per base, stranded: cells > 0
            one, _ = ce.ends(orc, rg, 1, 1, True, shift=shift, mapqual=3)
            every, _ = ce.ends(orc, rg, HUGE, 1, True, shift=shift, mapqual=3)
            assert np.array_equal(one, (every > 0).astype(np.int64))
    assert seen_capped > 20


def cols_part(cols):
    """merge_sorted's input form of sorted columns"""
    ref_off = np.asarray(cols["ref_off"], np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    part = {k: np.asarray(cols[k], np.int64) for k in ("pos", "end", "flag", "mapq")}
    part["rid"] = rid
    part["tlen"] = np.asarray(cols["tlen"], np.int64) if "tlen" in cols else np.zeros(len(rid), np.int64)
    return part


@pytest.mark.parametrize("L", [1, 40, 200, 5000])
def test_coverage_with_a_huge_cap_is_the_resized_coverage(L):
    for seed in (5, 6):
        cols, rg = _small(seed)
        for binsize, ss in ((1, False), (1, True), (50, False), (7, True)):
            want, woff = rz.coverage(rz.resize_columns(cols, L), rg, binsize, ss, mapqual=3)
            got, goff = ce.coverage(cols, rg, HUGE, L, binsize, ss, mapqual=3)
            assert np.array_equal(goff, woff) and np.array_equal(got, want), (seed, L, binsize, ss)
            assert got.sum() > 0


def test_planted_piles_have_the_answers_worked_out_by_hand():
    """reference of 10,000 bases; range A = [1000, 1100) '+', range B the same bases '-', range C = [0, 50) '+'.
    forward piles: 5 on base 1010, 9 on base 0, 4 on base 990 (10 bases in front of A); reverse piles: 6 ending on base 1020,
    3 ending on base 1139 (L - 1 = 39 bases behind A for L = 40)."""
    parts = [ce.planted(5, 0, 1010), ce.planted(9, 0, 0), ce.planted(4, 0, 990), ce.planted(6, 0, 1020, reverse=True),
             ce.planted(3, 0, 1139, reverse=True)]
    cols = ce.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([10_000], np.int64)
    rg = dict(rid=np.zeros(3, np.int32), loc=np.asarray([1000, 1000, 0], np.int32), len=np.asarray([100, 100, 50], np.int32),
              strand=np.asarray([1, -1, 1], np.int32))
    # ends, k = 2, per base with strands
    got, off = ce.ends(cols, rg, 2, 1, True)
    a, b, c = (_rows(got, off, i, True) for i in range(3))
    want_a = np.zeros((2, 100), np.int64)
    want_a[0, 10], want_a[1, 20] = 2, 2
    assert np.array_equal(a, want_a)
    want_b = np.zeros((2, 100), np.int64)              # mirrored: base 1010 is cell 89, 1020 is cell 79; the strands swap
    want_b[1, 89], want_b[0, 79] = 2, 2
    assert np.array_equal(b, want_b)
    assert c[0, 0] == 2 and c.sum() == 2                # the forward pile on base 0
    # counts: k = 2 gives 2 + 2 per range A, k = 100 all 11; without strands the cap is still per strand
    for k, want in ((2, [4, 4, 2]), (5, [10, 10, 5]), (100, [11, 11, 9])):
        cnt, _ = ce.ends(cols, rg, k, -1, False)
        assert cnt.tolist() == want
        cnt2, _ = ce.ends(cols, rg, k, -1, True)
        assert cnt2.reshape(-1, 2).sum(axis=1).tolist() == want
    assert ce.ends(cols, rg, 2, -1, True)[0].tolist() == [2, 2, 2, 2, 2, 0]
    # coverage, L = 40, k = 2: over A the pile on 990 covers 990 .. 1029 -> cells 0 .. 29 (2 kept), the pile on 1010 covers
    # cells 10 .. 49 (2), the reverse pile on 1020 covers 981 .. 1020 -> cells 0 .. 20 (2), the one on 1139 covers 1100 .. 1139:
    # the first base behind A -- nothing; L = 41 reaches cell 99
    cov, off = ce.coverage(cols, rg, 2, 40, 1, True)
    a = _rows(cov, off, 0, True)
    want = np.zeros((2, 100), np.int64)
    want[0, 0:30] += 2
    want[0, 10:50] += 2
    want[1, 0:21] += 2
    assert np.array_equal(a, want)
    assert np.array_equal(_rows(cov, off, 1, True), want[::-1, ::-1])
    a41 = _rows(ce.coverage(cols, rg, 2, 41, 1, True)[0], ce.coverage(cols, rg, 2, 41, 1, True)[1], 0, True)
    assert a41[1, 99] == 2 and a41[1, 98] == 0
    # range C: the forward pile on base 0 covers cells 0 .. 39, k = 2 of 9 kept; unstranded and in bins of 25
    c = _rows(*ce.coverage(cols, rg, 2, 40, 25, False), 2, False) if False else None
    flat, off = ce.coverage(cols, rg, 2, 40, 25, False)
    assert flat[off[2]:off[3]].tolist() == [50, 30]
    flat, off = ce.coverage(cols, rg, 100, 40, 25, False)
    assert flat[off[2]:off[3]].tolist() == [225, 135]


# ---- planmath.h through its own driver ---------------------------------------------------------------------------------------
DRIVER = os.path.join(ROOT, "tests", "asan", "cappedmath_driver")


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bamsignals_amd", "csrc"), "cappedmath"])

    def run(text):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([DRIVER], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        return [[int(v) for v in line.split()] for line in p.stdout.splitlines()]
    return run


def test_bins_a_tile_touches(driver):
    assert driver("binsize -1 binsize 1 binsize 7 binsize 65536") == [[HUGE], [1], [7], [65536]]
    cases = [(t, b) for t in (16, 64, 100, 2047, 2048) for b in (1, 2, 3, 7, 50, 63, 64, 65, 200, 2047, 2048, 2049, 100_000)]
    cases.append((2048, HUGE))
    got = driver(" ".join(f"tilebins {t} {b}" for t, b in cases))
    for (t, b), (n_acc, most) in zip(cases, got):
        if b == 1:
            assert n_acc == 0
            continue
        assert n_acc == (t - 1) // b + 2
        # the rule holds for every c0 the driver tried, and is no more than one accumulator generous
        assert most <= n_acc <= most + 1, (t, b)
        if b <= 2048:
            assert most == -(-(t - 1) // b) + 1 if (t - 1) % b else most >= (t - 1) // b + 1


def _widen(loc, w, L):
    if w <= 0:
        return [1, loc, 0, 0]
    lo = max(loc - (L - 1), 0)
    lead = loc - lo
    wide = lead + w + L - 1
    if wide > HUGE or lo + wide > HUGE:
        return [0, loc, 0, 0]
    return [1, lo, wide, lead] if wide > 0 else [1, loc, 0, lead]


def test_widened_and_clipped_ranges(driver):
    cases = [(100, 50, 40), (39, 50, 40), (38, 50, 40), (0, 50, 40), (-20, 90, 40), (5, 10, 1), (5, 0, 40), (7, 3, 1 << 24),
             (-200, 50, 40), (-88, 50, 40), (-89, 50, 40),
             # at the limit and one past it: the widened range ends on 2^31 - 1, then one beyond
             (HUGE - 600, 501, 100), (HUGE - 600, 502, 100), (0, HUGE - 99, 100), (0, HUGE - 98, 100)]
    got = driver(" ".join(f"widen {a} {b} {c}" for a, b, c in cases))
    assert got == [_widen(*c) for c in cases]
    assert [g[0] for g in got[-4:]] == [1, 0, 1, 0]
    # clipped exactly where base 0 is reached
    assert got[1] == [1, 0, 39 + 50 + 39, 39] and got[2] == [1, 0, 38 + 50 + 39, 38]
    # the window sums' indexes: the row's first and last pair are the first and last index read, none behind the row
    assert got[4] == [1, 0, 90 - 20 + 39, -20] and got[8] == [1, -200, 0, -200] and got[9] == [1, 0, 1, -88] and got[10][2] == 0
    for loc, w, L in cases[:4]:
        fits, lo, wide, lead = _widen(loc, w, L)
        idx = driver(" ".join(f"window {u} {lead} {L}" for u in (0, w - 1)))
        assert idx[0] == [lead, lead - L, lead + L - 1, lead - 1]
        assert idx[1][2] == wide - 1 and max(idx[1]) == wide - 1


def test_tiles_are_per_base_whatever_the_results_bins(driver):
    # three ranges, the result laid out in bins of 50 with strands (2 * ceil(w / 50) cells a range)
    rg = [(100, 130, 1), (500, 0, 1), (900, 64, -1)]
    off = np.concatenate([[0], np.cumsum([2 * -(-w // 50) for _, w, _ in rg])]).tolist()
    text = "tiles 64 3 " + " ".join(f"{a} {w} {s} {o}" for (a, w, s), o in zip(rg, off)) + f" {off[-1]}"
    got = driver(text)
    assert got[0] == [4]
    assert got[1:] == [[100, 130, 0, 64, 0, 0], [100, 130, 64, 64, 0, 0], [100, 130, 128, 2, 0, 0], [900, 64, 0, 64, off[2], 1]]
