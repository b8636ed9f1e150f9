"""GPU: the per-range summaries (bsig_plan_create_summary, k_summary_tiles / k_summary_finish; bamSummary) against the
definition -- sum, max, first argmax and counts of the C oracle's per-base cells, range by range
(tests/summary_expected.py).  All exact.

The refusal for a range whose sum could pass 2^63 is not exercised: no input a test can hold reaches it."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import depthhist_expected as de
import summary_expected as se
from test_depthhist_gpu import (MORE, REF_LEN, VARIANTS, _cat, _params, _pe_kw, _pile, _ranges, _upload,  # noqa: F401
                                decode_mode, fixture, synth)
from test_summary_cpu import PARAM_RULE

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
THRS = ((), (1,), (1, 2, 3, 5, 8, 13, 21, 34))
LONG = THRS[2]


def _run(ctx, reads, rg, signal, ss, thr, runs=2, **kw):
    """a plan's first run (fused lookups) and its later ones (windows kept), which must agree; (result, stats, runs)"""
    from bamsignals_amd.device import SummaryPlan
    plan = SummaryPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(signal, ss, **kw), thr)
    try:
        n, S = len(rg["len"]), 2 if ss else 1
        assert plan.cells == n * S * (3 + len(thr))
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int64 and got[0].shape == (n, S, 3 + len(thr))
        return got[0], plan.stats(), plan.runs
    finally:
        plan.close()


def _diff(got, want):
    bad = np.argwhere(got != want)[:6]
    return [(tuple(b), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad]


def _check(ctx, reads, cells, rg, signal, ss, thr, runs=2, **kw):
    """cells: the oracle's cells of these ranges and parameters (computed once, shared among the thresholds)"""
    got, st, n_runs = _run(ctx, reads, rg, signal, ss, thr, runs=runs, **kw)
    want = se.from_cells(cells, rg, ss, thr)
    assert np.array_equal(got, want), (signal, ss, thr, kw, _diff(got, want))
    assert st["cells"] == got.size
    return got, st, n_runs


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [None, "64"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_grid(synth, variant, heavy, monkeypatch):
    """every width of a signal's row; once more with the ceiling lowered so that nearly every tile takes the 32-bit image"""
    ctx, cols, reads, orc = synth
    signal, ss, kw = VARIANTS[variant]
    if heavy:
        monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", heavy)
    some_max = some_tie = some_step = False
    for w in (1, 100, 2048, 2049, 10_000):
        rg = _ranges(60 if w < 10_000 else 12, w, seed=w)
        assert w >= 10_000 or len(set(rg["strand"].tolist())) == 3
        cells = de.cells(orc, rg, signal, ss, **kw)
        rows = se.rows_of(cells, rg, ss)
        want = se.from_rows(rows, LONG)
        # (not vacuous, on the expected side first)
        some_max |= bool(want[..., 1].max() > 0)
        some_tie |= se.has_tie(rows)
        some_step |= bool((want[..., 3] != want[..., -1]).any())
        for thr in THRS:
            got, st, n_runs = _check(ctx, reads, cells, rg, signal, ss, thr, **kw)
            assert (st["heavy_tiles"] == 0) if not heavy else (w < 2048 or st["heavy_tiles"] > 0)
            assert n_runs >= st["heavy_tiles"]
    assert some_max and some_tie and some_step


@pytest.mark.parametrize("variant", sorted(MORE))
def test_filters_and_the_midpoint_rule(synth, variant):
    ctx, cols, reads, orc = synth
    signal, ss, kw = MORE[variant]
    rg = _ranges(40, 3000, seed=5, jitter=800)
    cells = de.cells(orc, rg, signal, ss, **kw)
    assert cells.sum() > 1000
    for thr in ((2, 4), LONG):
        _check(ctx, reads, cells, rg, signal, ss, thr, **kw)


# ---- seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,w", [(64, 64 * 3 + 17), (0, 2048 * 2 + 100)])
def test_seams(synth, tile, w):
    """EQUAL maxima on the last cell of one tile and the first of the next, and on cell 0 and cell w - 1 (cells in range
    orientation: a '-' range's tiles are cut from its other end), with lower piles around them; the first one wins"""
    ctx = synth[0]
    loc = 40_000
    step = tile or 2048
    for strand in (1, -1):
        def g(x):
            return loc + x if strand > 0 else loc + w - 1 - x
        for deck, tied in (("seam", (step - 1, step)), ("seam2", (2 * step - 1, 2 * step)), ("ends", (0, w - 1)),
                           ("all", (0, step - 1, step, w - 1))):
            parts = []
            # (one-base reads: a pile is one cell of coverage as well, so neighbouring piles stay equal)
            for x in tied:
                parts += [de.planted(5, 0, g(x), read_len=1), de.planted(5, 0, g(x), reverse=True, read_len=1)]
            for x in (7, step + 9, w - 30):
                parts += [de.planted(2, 0, g(x), read_len=1), de.planted(3, 0, g(x), reverse=True, read_len=1)]
            cols = de.merge_sorted(parts, 1)
            cols["ref_len"] = np.asarray([200_000], np.int64)
            reads = _upload(ctx, cols)
            try:
                rg = dict(rid=[0], loc=[loc], len=[w], strand=[strand])
                for signal, ss in (("coverage", False), ("ends", False), ("ends", True)):
                    cells = de.cells(cols, rg, signal, ss)
                    rows = se.rows_of(cells, rg, ss)
                    want = se.from_rows(rows, (1, 5, 10))
                    # (the planting took: the tied cells hold the maximum, and the first of them is the summit)
                    for r in range(rows[0].shape[0]):
                        assert all(rows[0][r][x] == rows[0][r].max() > 0 for x in tied), (deck, signal, ss, strand)
                        assert want[0, r, 2] == min(tied)
                    for threads in (64, 256):
                        got, st, _ = _check(ctx, reads, cells, rg, signal, ss, (1, 5, 10), tile_cells=tile, threads=threads)
                        assert st["n_items"] == (w + step - 1) // step and st["heavy_tiles"] == 0
            finally:
                reads.close()


# ---- run boundaries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["cov", "ends-ss"])
def test_run_boundaries(synth, variant, monkeypatch):
    """many ranges per run (a flush at every tile) and one range over many runs (combined with atomics), whatever the cut"""
    ctx, cols, reads, orc = synth
    signal, ss, kw = VARIANTS[variant]
    rng = np.random.default_rng(17)
    n = 200
    small = dict(rid=rng.integers(0, 2, n), loc=rng.integers(1000, 690_000, n), len=rng.integers(1, 51, n),
                 strand=rng.integers(-1, 2, n))
    whole = dict(rid=[1], loc=[0], len=[REF_LEN[1]], strand=[-1])
    empty = dict(rid=[0, 1, 0], loc=[500, 90_000, 300_000], len=[0, 0, 0], strand=[1, -1, 0])
    dup = {k: np.asarray(v)[[3, 3, 77, 3]] for k, v in small.items()}
    rg = _cat(small, empty, whole, dup, dict(rid=[1], loc=[0], len=[REF_LEN[1]], strand=[1]))
    cells = de.cells(orc, rg, signal, ss, **kw)
    results, counts = {}, {}
    for per in ("1", "1000000", None):
        if per:
            monkeypatch.setenv("BAMSIGNALS_SUMMARY_RUN_TILES", per)
        else:
            monkeypatch.delenv("BAMSIGNALS_SUMMARY_RUN_TILES")
        results[per], st, counts[per] = _check(ctx, reads, cells, rg, signal, ss, LONG, **kw)
    assert np.array_equal(results["1"], results["1000000"]) and np.array_equal(results["1"], results[None])
    tiles = 204 + 2 * ((REF_LEN[1] + 2047) // 2048)
    assert st["n_items"] == tiles == counts["1"] and counts["1000000"] == 1 and 1 < counts[None] <= tiles
    got = results[None]
    assert (got[200:203, :, 2] == -1).all() and not got[200:203, :, :2].any() and not got[200:203, :, 3:].any()
    assert np.array_equal(got[204], got[3]) and np.array_equal(got[205], got[3]) and np.array_equal(got[206], got[77])
    assert got[203, :, 1].max() > 2 and got[203, :, 0].sum() == got[208, :, 0].sum()


# ---- the thresholds' edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [7, 100])
def test_threshold_edges(synth, t):
    """piles of exactly t - 1, t and t + 1 reads on one base"""
    ctx = synth[0]
    parts = [de.planted(t - 1, 0, 50_000), de.planted(t, 0, 50_500), de.planted(t + 1, 0, 51_000),
             de.planted(t - 1, 0, 52_000, reverse=True), de.planted(t + 1, 0, 52_500, reverse=True)]
    cols = de.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=[0, 0], loc=[49_000, 50_400], len=[5000, 300], strand=[1, -1])
        for signal, ss in (("coverage", False), ("ends", False), ("ends", True)):
            cells = de.cells(cols, rg, signal, ss)
            per = 40 if signal == "coverage" else 1
            thr = (t - 1, t, t + 1, t + 2)
            want = se.from_cells(cells, rg, ss, thr)
            # range 0 sees all five piles, range 1 the pile of t alone
            assert want[0, :, 3:].sum(axis=0).tolist() == [5 * per, 3 * per, 2 * per, 0]
            assert want[1, :, 3:].sum(axis=0).tolist() == [per, per, 0, 0] and want[:, :, 1].max() == t + 1
            got, _, _ = _check(ctx, reads, cells, rg, signal, ss, thr)
    finally:
        reads.close()


# ---- 16-bit -> wide --------------------------------------------------------------------------------------------------
def _with_neighbours(rg):
    """_pile's ranges and one whose wide tile has ordinary tiles on both sides of it"""
    return _cat(rg, dict(rid=[0], loc=[47_500], len=[6000], strand=[-1]))


@pytest.mark.parametrize("n", [32_766, 32_767, 32_768, 32_769])
@pytest.mark.parametrize("beside", [False, True])
def test_coverage_piles_around_the_16_bit_ceiling(synth, n, beside):
    ctx = synth[0]
    cols, reads, rg = _pile(ctx, n, beside)
    rg = _with_neighbours(rg)
    try:
        cells = de.cells(cols, rg, "coverage", False)
        thr = (1, 32_767, 32_768)
        got, st, _ = _check(ctx, reads, cells, rg, "coverage", False, thr)
        assert (got[:, 0, 1] >= n).all()
        assert (st["heavy_tiles"] > 0) == (n + (3000 if beside else 0) > 32_767), st["heavy_tiles"]
        assert st["n_items"] == 2 + 1 + 3
    finally:
        reads.close()


@pytest.mark.parametrize("n", [32_768, 65_535, 65_536, 65_537])
@pytest.mark.parametrize("beside", [False, True])
def test_end_piles_around_and_past_16_bits(synth, n, beside):
    ctx = synth[0]
    for reverse in (False, True):
        cols, reads, rg = _pile(ctx, n, beside, reverse=reverse)
        rg = _with_neighbours(rg)
        try:
            for ss in (False, True):
                cells = de.cells(cols, rg, "ends", ss)
                thr = (1, 32_768, 65_535, 65_536)
                got, st, _ = _check(ctx, reads, cells, rg, "ends", ss, thr, runs=1)
                assert (got[:, :, 1].max(axis=1) >= n).all()
                assert (st["heavy_tiles"] > 0) == (n + (3000 if beside else 0) > 32_768), st["heavy_tiles"]
        finally:
            reads.close()


# ---- packed forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"BAMSIGNALS_PACKED_HALF": "0"}, {"BAMSIGNALS_PACK": "0"}])
def test_packed_forms(synth, env, monkeypatch):
    ctx, cols, _, orc = synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads = _upload(ctx, cols)
    rg = _ranges(80, 2500, seed=11)
    try:
        for signal, ss, kw in list(VARIANTS.values()) + [MORE["ends-ss-midpoint"]]:
            cells = de.cells(orc, rg, signal, ss, **kw)
            got, st, _ = _check(ctx, reads, cells, rg, signal, ss, (1, 3), **kw)
            assert got[..., 0].sum() > 0
            if env.get("BAMSIGNALS_PACK") == "0":
                assert st["visits_packed"] == 0
            else:
                half = signal == "ends" and not kw and not env
                assert st["visits_packed"] > 0 and st["bytes_per_visit_packed"] == (2 if half else 8 if "tlen_filter" in kw else 4)
    finally:
        reads.close()


# ---- edges and order -------------------------------------------------------------------------------------------------
def test_edges(synth):
    ctx, cols, reads, orc = synth
    for signal, ss, kw in VARIANTS.values():
        S = 2 if ss else 1
        got, st, n_runs = _run(ctx, reads, dict(rid=[], loc=[], len=[], strand=[]), signal, ss, (1, 2), **kw)
        assert got.shape == (0, S, 5) and st["n_items"] == 0 and n_runs == 0
        got, st, n_runs = _run(ctx, reads, dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1]), signal, ss, (1, 2), **kw)
        assert got.tolist() == [[[0, 0, -1, 0, 0]] * S] * 2 and n_runs == 0
        # wholly outside the reference (behind the reads that hang over its end), and over both of its ends
        rg = dict(rid=[0, 1, 1], loc=[-500, 705_017, -300], len=[400, 100, REF_LEN[1] + 900], strand=[1, -1, -1])
        got, _, _ = _check(ctx, reads, de.cells(orc, rg, signal, ss, **kw), rg, signal, ss, (1, 2), **kw)
        assert got[:2].tolist() == [[[0, 0, 0, 0, 0]] * S] * 2 and got[2, :, 0].sum() > 0


def test_a_shuffled_deck_gives_the_shuffled_rows(synth):
    ctx, cols, reads, orc = synth
    rg = _cat(_ranges(50, 3000, seed=3, jitter=2900), dict(rid=[0, 1], loc=[70, 80], len=[0, 5000], strand=[1, -1]))
    perm = np.random.default_rng(8).permutation(len(rg["len"]))
    shuffled = {k: v[perm] for k, v in rg.items()}
    for signal, ss, kw in VARIANTS.values():
        a, _, _ = _check(ctx, reads, de.cells(orc, rg, signal, ss, **kw), rg, signal, ss, (1, 4), **kw)
        b, _, _ = _run(ctx, reads, shuffled, signal, ss, (1, 4), runs=1, **kw)
        assert np.array_equal(b, a[perm]) and len(np.unique(a[:, 0, 0])) > 20


# ---- plans -----------------------------------------------------------------------------------------------------------
def test_stale_plan_and_wrong_run_calls(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, HistPlan, Plan, SumPlan, SummaryPlan, XcorrPlan, make_params
    ctx, cols, _, _ = synth
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        a = ([0], [10], [100], [1])
        prof = make_params(_lib.MODE_PROFILE)
        mp = SummaryPlan(ctx, reads, *a, _params("coverage", False), (1, 5))
        me = SummaryPlan(ctx, reads, *a, _params("ends", True), ())
        pp, sp, xp = Plan(ctx, reads, *a, prof), SumPlan(ctx, reads, *a, prof), XcorrPlan(ctx, reads, *a, prof, 20)
        fp = FragPlan(ctx, reads, *a, make_params(_lib.MODE_COUNT, tlen_filter=(0, 24), binsize=-1, requiredF=66), 1)
        hp = HistPlan(ctx, reads, *a, _params("coverage", False), 24)
        b32, b64 = np.zeros(400, np.int32), np.zeros(400, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        host, dev = "a summary plan runs with bsig_plan_run_summary_host", "a summary plan runs with bsig_plan_run_summary"
        for fn, plan, buf, says in (
                (lib.bsig_plan_run_host, mp, p32, host),
                (lib.bsig_plan_run, mp, p32, dev),
                (lib.bsig_plan_run_host_async, mp, p32, dev),
                (lib.bsig_plan_run_sum_host, mp, p64, host),
                (lib.bsig_plan_run_sum, mp, p64, dev),
                (lib.bsig_plan_run_xcorr_host, me, p64, host),
                (lib.bsig_plan_run_xcorr, me, p64, dev),
                (lib.bsig_plan_run_frag_host, mp, p64, host),
                (lib.bsig_plan_run_frag, mp, p64, dev),
                (lib.bsig_plan_run_hist_host, me, p64, host),
                (lib.bsig_plan_run_hist, mp, p64, dev),
                (lib.bsig_plan_run_summary_host, pp, p64, "not a summary plan: bsig_plan_run_host runs it"),
                (lib.bsig_plan_run_summary, pp, p64, "not a summary plan: bsig_plan_run runs it"),
                (lib.bsig_plan_run_summary_host, sp, p64, "not a summary plan: bsig_plan_run_sum_host runs it"),
                (lib.bsig_plan_run_summary, sp, p64, "not a summary plan: bsig_plan_run_sum runs it"),
                (lib.bsig_plan_run_summary_host, xp, p64, "not a summary plan: bsig_plan_run_xcorr_host runs it"),
                (lib.bsig_plan_run_summary, xp, p64, "not a summary plan: bsig_plan_run_xcorr runs it"),
                (lib.bsig_plan_run_summary_host, fp, p64, "not a summary plan: bsig_plan_run_frag_host runs it"),
                (lib.bsig_plan_run_summary, fp, p64, "not a summary plan: bsig_plan_run_frag runs it"),
                (lib.bsig_plan_run_summary_host, hp, p64, "not a summary plan: bsig_plan_run_hist_host runs it"),
                (lib.bsig_plan_run_summary, hp, p64, "not a summary plan: bsig_plan_run_hist runs it")):
            assert fn(plan._h, buf) == -1
            assert lib.bsig_last_error().decode() == says
        assert not b32.any() and not b64.any()
        h = C.c_void_p()
        assert lib.bsig_plan_runs_create(mp._h, C.byref(h)) == -1
        assert lib.bsig_last_error().decode() == "a summary plan has no per-range result to encode"
        for other in (pp, sp, xp, fp, hp):
            assert lib.bsig_plan_summary_cells(other._h) == 0 and lib.bsig_plan_summary_runs(other._h) == 0
        assert lib.bsig_plan_summary_cells(mp._h) == 5 and lib.bsig_plan_summary_cells(me._h) == 6
        assert lib.bsig_plan_summary_cells(None) == 0 and lib.bsig_plan_summary_runs(None) == 0 and lib.bsig_plan_summary_runs(mp._h) == 1
        assert lib.bsig_plan_hist_cells(mp._h) == 0 and lib.bsig_plan_sum_cells(mp._h) == 0 and lib.bsig_plan_frag_cells(mp._h) == 0
        first = mp.run_host()
        assert first.shape == (1, 1, 5) and first[0, 0, 0] > 0 and first[0, 0, 3] >= first[0, 0, 4]
        assert np.array_equal(mp.run_host(), first) and np.array_equal(mp.run_host(), first)
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        with pytest.raises(_lib.BsigError, match="make a new plan"):
            mp.run_host()
        mp2 = SummaryPlan(ctx, reads, *a, _params("coverage", False), (1, 5))
        assert np.array_equal(mp2.run_host(), first)
        for p in (mp, mp2, me, pp, sp, xp, fp, hp):
            p.close()
    finally:
        reads.close()


def test_errors(synth):
    """the parameter rule's table (tests/test_summary_cpu.py) and what only the plan call can express"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import SummaryPlan, make_params
    ctx, cols, reads, _ = synth
    lib = _lib.load()
    a = ([0], [10], [100], [1])
    for kw, code, message in PARAM_RULE:
        kw = dict(kw)
        tf = kw.get("tlen_filter", ())
        p = _lib.Params()
        p.mode, p.binsize, p.filteredF = (_lib.MODE_COVERAGE if kw["signal"] == "coverage" else _lib.MODE_PROFILE), 1, -1
        p.ss, p.tspan, p.pe_mid = kw.get("ss", 0), kw.get("tspan", 0), kw.get("pe_mid", 0)
        p.n_tlen_filter = len(tf)
        for i, v in enumerate(tf):
            p.tlen_filter[i] = v
        thr = kw.get("thresholds", (1, 10))
        if kw.get("null"):
            rid, loc, ln, strand = (np.asarray(x, np.int32) for x in a)
            h = C.c_void_p()
            rc = lib.bsig_plan_create_summary(ctx._h, reads._h, 1, rid.ctypes.data, loc.ctypes.data, ln.ctypes.data,
                                              strand.ctypes.data, C.byref(p), len(thr), None, C.byref(h))
            assert (rc, lib.bsig_last_error().decode()) == (code, message) and not h.value
            continue
        with pytest.raises(_lib.BsigError) as e:
            SummaryPlan(ctx, reads, *a, p, thr)
        assert (e.value.code, str(e.value)) == (code, message)
    for p, message in (
            (make_params(_lib.MODE_COUNT, binsize=-1), "the range summary reduces per-base cells: bamCount has one cell per range"),
            (make_params(_lib.MODE_COVERAGE_EX), "the range summary of coverage is per base and unstranded: mode BSIG_MODE_COVERAGE"),
            (make_params(_lib.MODE_PROFILE, binsize=2), "the range summary is per base: binsize must be 1"),
            (make_params(_lib.MODE_PROFILE, shift=1), "the range summary reduces unshifted positions: shift must be 0"),
            (make_params(_lib.MODE_COVERAGE, shift=-1), "the range summary reduces unshifted positions: shift must be 0"),
            (make_params(_lib.MODE_COVERAGE, ss=True), "the range summary of coverage has no strands: ss must be 0"),
            (make_params(_lib.MODE_PROFILE, threads=96), "threads must be 64, 128 or 256"),
            (make_params(_lib.MODE_COVERAGE, tile_cells=8), "tile_cells must be between 16 and 2048"),
            (make_params(_lib.MODE_PROFILE, tile_cells=2049), "tile_cells must be between 16 and 2048"),
            (make_params(7), "unknown mode 7")):
        with pytest.raises(_lib.BsigError) as e:
            SummaryPlan(ctx, reads, *a, p, (1,))
        assert (e.value.code_name, str(e.value)) == ("BSIG_ERR_ARG", message)
    with pytest.raises(_lib.BsigError) as e:
        SummaryPlan(ctx, reads, [5], [10], [100], [1], _params("coverage", False), (1,))
    assert e.value.code_name == "BSIG_ERR_CHROM"
    with pytest.raises(_lib.BsigError, match="negative width") as e:
        SummaryPlan(ctx, reads, [0], [10], [-1], [1], _params("ends", True), (1,))
    assert e.value.code_name == "BSIG_ERR_ARG"
    # the edges of what is allowed
    for tile, thr in ((16, ()), (2048, (1, 2, 3, 4, 5, 6, 7, 2 ** 31 - 1))):
        SummaryPlan(ctx, reads, *a, _params("ends", True, tile_cells=tile), thr).close()


# ---- file level ------------------------------------------------------------------------------------------------------
def _as_summary(want, ss):
    return want if ss else want[:, 0, :]


def test_file_level(fixture, decode_mode):
    from bamsignals_amd import RangeSummary, bamCoverage, bamDepthHist, bamSummary
    gr, rg, cols, whole, whole_rg = fixture
    orc = de.oracle_reads(cols)
    thr = (1, 2, 5, 20)
    for signal, choices in (("coverage", ("ignore", "extend")), ("ends", ("ignore", "filter", "midpoint"))):
        for pe in choices:
            for ss in ((False,) if signal == "coverage" else (True, False)):
                want = _as_summary(se.expected(orc, rg, signal, ss, thr, **_pe_kw(signal, pe)), ss)
                rs = bamSummary(BAM, gr, thresholds=thr, signal=signal, ss=ss, paired_end=pe, verbose=False)
                assert isinstance(rs, RangeSummary) and rs.thresholds == thr and rs.sum.dtype == np.int64
                assert rs.sum.shape == ((50, 2) if ss else (50,)) and rs.covered.shape == rs.sum.shape + (4,)
                assert np.array_equal(rs.sum, want[..., 0]) and np.array_equal(rs.max, want[..., 1]), (signal, pe, ss)
                assert np.array_equal(rs.summit, want[..., 2]) and np.array_equal(rs.covered, want[..., 3:]), (signal, pe, ss)
                assert np.array_equal(rs.width, rg["len"]) and rs.sum.sum() > 0
    rs = bamSummary(BAM, gr, thresholds=(), mapqual=30, filteredFlag=1024, verbose=False)
    per_base = bamCoverage(BAM, gr, mapqual=30, filteredFlag=1024, verbose=False)
    assert rs.sum.tolist() == [int(np.asarray(s, np.int64).sum()) for s in per_base]
    assert rs.max.tolist() == [int(np.max(s)) for s in per_base] and rs.summit.tolist() == [int(np.argmax(s)) for s in per_base]
    # whole chromosomes: the per-base coverage peaks at 208 / 184 / 199, the per-strand 5'-end piles at 11 / 9 / 10
    rc = bamSummary(BAM, whole, thresholds=(1, 20, 100), verbose=False)
    assert rc.max.tolist() == [208, 184, 199]
    cov = bamCoverage(BAM, whole, verbose=False)
    assert rc.sum.tolist() == [int(np.asarray(s, np.int64).sum()) for s in cov]
    assert rc.summit.tolist() == [int(np.argmax(s)) for s in cov]
    dh = bamDepthHist(BAM, whole, maxdepth=255, verbose=False)
    for k, t in enumerate((1, 20, 100)):
        assert int(rc.covered[:, k].sum()) == int(dh.counts[t:].sum()) > 0
    re_ = bamSummary(BAM, whole, thresholds=(1, 2), signal="ends", ss=True, verbose=False)
    assert re_.max.max(axis=1).tolist() == [11, 9, 10]
    de_ = bamDepthHist(BAM, whole, maxdepth=12, signal="ends", verbose=False)
    assert int(re_.covered[..., 1].sum()) == int(de_.counts[2:].sum()) > 0 and int(re_.sum.sum()) == de_.total


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import _lib, bamSummary
    from bamsignals_amd.wrappers import last_call_route
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        for kw in (dict(signal="coverage", paired_end="extend"), dict(signal="ends", ss=True, paired_end="midpoint")):
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
            one = bamSummary(BAM, gr, verbose=False, **kw)
            assert "1 GPU slot(s)" in last_call_route() and "summary" in last_call_route()
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
            four = bamSummary(BAM, gr, verbose=False, **kw)
            assert "4 GPU slot(s)" in last_call_route() and "rows placed on the host" in last_call_route()
            for name in ("sum", "max", "summit", "covered"):
                assert np.array_equal(getattr(one, name), getattr(four, name)), name
            assert one.sum.any() and one.covered.any()
    finally:
        _lib.load().bsig_cache_clear()


# ---- the use ---------------------------------------------------------------------------------------------------------
def test_peaks_and_failing_targets_are_read_off_the_data(synth, tmp_path):
    """the synthetic background plus 30 planted peaks: a plateau of 300 + i forward reads of 40 bases and, on one base of
    it, 60 one-base reads -- the summit.  Even peaks sit in narrow targets (44 bases), odd ones in targets of 2,000."""
    from bamsignals_amd import GRanges, _lib, bamCoverage, bamSummary, write_columns_as_bam
    ctx, bg, _, orc_bg = synth
    ref_off = np.asarray(bg["ref_off"])
    rng = np.random.default_rng(12)
    n = 30
    rid = np.arange(n) % 2
    start = 20_000 + 20_000 * np.arange(n)                       # the plateau's first base (0-based)
    spike = start + rng.integers(0, 40, n)
    width = np.where(np.arange(n) % 2 == 0, 44, 2000)
    loc = start - np.where(np.arange(n) % 2 == 0, 2, rng.integers(100, 1900, n))
    strand = np.where(rng.random(n) < 0.5, 1, -1)
    parts = [dict(rid=np.repeat(np.arange(2), np.diff(ref_off)), pos=bg["pos"], end=bg["end"], flag=bg["flag"], mapq=bg["mapq"],
                  tlen=bg["tlen"])]
    for i in range(n):
        parts.append(de.planted(300 + i, 150, start[i], rid=rid[i]))
        parts.append(de.planted(60, 150, spike[i], rid=rid[i], read_len=1))
    cols = de.merge_sorted(parts, 2)
    cols["ref_len"] = np.asarray(REF_LEN, np.int64)
    rg = dict(rid=rid, loc=loc, len=width, strand=strand)
    bg_max = int(de.cells(orc_bg, rg, "coverage", False).max())
    assert bg_max < 60                                           # (the spike is the summit whatever lies under it)
    bam = str(tmp_path / "peaks.bam")
    cig = dict(cigar_off=np.arange(len(cols["pos"]) + 1, dtype=np.int64),
               cigar=((cols["end"].astype(np.int64) - cols["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(bam, ["chrA", "chrB"], dict(cols, **cig))
    try:
        gr = GRanges([("chrA", "chrB")[r] for r in rid], loc + 1, width=width, strand=["+" if s > 0 else "-" for s in strand])
        rs = bamSummary(bam, gr, thresholds=(20, 300), verbose=False)
        assert rs.summit_position().tolist() == (spike + 1).tolist()
        assert (rs.max >= 360 + np.arange(n)).all() and (rs.max <= 360 + np.arange(n) + bg_max).all()
        assert (rs.covered[:, 1] == 40).all()
        per_base = bamCoverage(bam, gr, verbose=False)
        named = [i for i, c in enumerate(per_base) if 10 * int(np.count_nonzero(np.asarray(c) >= 20)) < 9 * len(c)]
        assert rs.failing(20, 0.9).tolist() == named and 0 < len(named) < n          # (some targets fail, some do not)
        assert rs.sum.tolist() == [int(np.asarray(c, np.int64).sum()) for c in per_base]
        # the 5' ends: the plateau's reads begin on `start`, forward -- the sense row of a '+' target, the antisense of a '-'
        re_ = bamSummary(bam, gr, thresholds=(), signal="ends", ss=True, verbose=False)
        row = np.where(strand > 0, 0, 1)
        assert re_.summit_position()[np.arange(n), row].tolist() == (start + 1).tolist()
        assert (re_.max[np.arange(n), row] >= 300 + np.arange(n)).all()
    finally:
        _lib.load().bsig_cache_clear()
