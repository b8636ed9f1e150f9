"""GPU: the scaled regions (bsig_plan_create_scaled, k_scaled_tiles; bamScaled) against the definition -- the C oracle's
per-base cells added into bin c * N // w, range by range (tests/scaled_expected.py).  All exact.

The refusal for a range whose sum could pass 2^63 is not exercised: no input a test can hold reaches it."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import depthhist_expected as de
import scaled_expected as sc
import summary_expected as se
from test_depthhist_gpu import (MORE, REF_LEN, VARIANTS, _cat, _params, _pe_kw, _pile, _ranges, _upload,  # noqa: F401
                                decode_mode, fixture, synth)
from test_scaled_cpu import PARAM_RULE
from test_summary_gpu import _with_neighbours

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
NS = (1, 7, 100, 2048)


def _run(ctx, reads, rg, signal, ss, N, runs=2, **kw):
    """a plan's first run (fused lookups) and its later ones (windows kept), which must agree; (result, stats, runs)"""
    from bamsignals_amd.device import ScaledPlan
    plan = ScaledPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(signal, ss, **kw), N)
    try:
        n, S = len(rg["len"]), 2 if ss else 1
        assert plan.cells == n * S * N
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int64 and got[0].shape == (n, S, N)
        return got[0], plan.stats(), plan.runs
    finally:
        plan.close()


def _diff(got, want):
    bad = np.argwhere(got != want)[:6]
    return [(tuple(b), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad]


def _check(ctx, reads, cells, rg, signal, ss, N, runs=2, **kw):
    """cells: the oracle's cells of these ranges and parameters (computed once, shared among the bin counts)"""
    got, st, n_runs = _run(ctx, reads, rg, signal, ss, N, runs=runs, **kw)
    want = sc.from_cells(cells, rg, ss, N)
    assert np.array_equal(got, want), (signal, ss, N, kw, _diff(got, want))
    assert st["cells"] == got.size
    return got, st, n_runs


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segmented", [None, "1"])
@pytest.mark.parametrize("heavy", [None, "64"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_grid(synth, variant, heavy, segmented, monkeypatch):
    """every width of a signal's row; once more with the ceiling lowered so that nearly every tile takes the 32-bit image;
    and both with the segmented consumer forced"""
    ctx, cols, reads, orc = synth
    signal, ss, kw = VARIANTS[variant]
    if heavy:
        monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", heavy)
    if segmented:
        monkeypatch.setenv("BAMSIGNALS_SCALED_SEGMENTED", segmented)
    some = empty_bins = ragged = False
    for w in (1, 100, 2048, 2049, 10_000):
        rg = _ranges(60 if w < 10_000 else 12, w, seed=w)
        assert w >= 10_000 or len(set(rg["strand"].tolist())) == 3
        cells = de.cells(orc, rg, signal, ss, **kw)
        for N in NS:
            # (not vacuous, on the expected side first)
            some |= bool(sc.from_cells(cells, rg, ss, N).any())
            empty_bins |= w < N
            ragged |= w % N != 0
            got, st, n_runs = _check(ctx, reads, cells, rg, signal, ss, N, **kw)
            assert (st["heavy_tiles"] == 0) if not heavy else (w < 2048 or st["heavy_tiles"] > 0)
            assert n_runs >= st["heavy_tiles"]
    assert some and empty_bins and ragged


@pytest.mark.parametrize("variant", sorted(MORE))
def test_filters_and_the_midpoint_rule(synth, variant):
    ctx, cols, reads, orc = synth
    signal, ss, kw = MORE[variant]
    rg = _ranges(40, 3000, seed=5, jitter=800)
    cells = de.cells(orc, rg, signal, ss, **kw)
    assert cells.sum() > 1000 and len(set(rg["len"].tolist())) > 10
    _check(ctx, reads, cells, rg, signal, ss, 64, **kw)


def test_stats_are_the_ordinary_plans(synth):
    from bamsignals_amd.device import Plan
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 5000, seed=2048)
    for signal, ss, kw in list(VARIANTS.values()) + [MORE["ends-ss-midpoint"]]:
        for tile in (2048, 512):
            got, st, _ = _run(ctx, reads, rg, signal, ss, 100, runs=1, tile_cells=tile, **kw)
            plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(signal, ss, tile_cells=tile, **kw))
            cs = plan.stats()
            plan.close()
            assert st["cells"] == 60 * (2 if ss else 1) * 100 and st["heavy_tiles"] == 0 and st["n_ranges"] == 60
            assert st["n_items"] == cs["n_items"] == 60 * ((5000 + tile - 1) // tile)
            for k in ("visits", "visits_packed", "visits_short", "bytes_per_visit_packed", "bytes_per_visit_short",
                      "bytes_per_visit_long"):
                assert st[k] == cs[k], (signal, ss, kw, k)
            assert st["visits"] > 0


def test_the_plans_own_choice_of_consumer(synth, monkeypatch):
    """the segmented consumer is the plan's own choice only for coverage whose cells lie mostly in ranges of w >= 256 N
    (a wave step of the coverage walk spans 256 cells); the variable forces either form; the integers do not depend on it"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import ScaledPlan, SummaryPlan
    ctx, cols, reads, orc = synth
    lib = _lib.load()
    monkeypatch.delenv("BAMSIGNALS_SCALED_SEGMENTED", raising=False)

    def deck(widths):
        n = len(widths)
        return dict(rid=np.zeros(n, np.int32), loc=(10_000 + 60_000 * np.arange(n)).astype(np.int32),
                    len=np.asarray(widths, np.int32), strand=np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int32))

    def form(rg, signal, ss, N):
        plan = ScaledPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(signal, ss), N)
        try:
            assert plan.segmented == bool(lib.bsig_plan_scaled_segmented(plan._h))
            return plan.segmented, plan.run_host()
        finally:
            plan.close()

    cases = [
        # (widths, N, coverage's own form)
        ([1000] * 20, 10, False),               # bins of 100 cells: every wave would take the scan
        ([1000] * 20, 3, True),                 # bins of 333 cells
        ([2560] * 5, 10, True),                 # bins of exactly 256
        ([2559] * 5, 10, False),
        ([10_000] * 12, 7, True),
        ([10_000] * 12, 100, False),
        ([1000] * 10 + [50_000] * 2, 100, True),        # 100,000 of 110,000 cells in wide bins
        ([1000] * 31 + [30_000], 100, False),           # 30,000 of 61,000: just under half
        ([1000] * 29 + [30_000], 100, True),            # 30,000 of 59,000: just over
        ([0, 0], 5, False),
    ]
    seen = set()
    for widths, N, want in cases:
        rg = deck(widths)
        monkeypatch.delenv("BAMSIGNALS_SCALED_SEGMENTED", raising=False)
        got, own = form(rg, "coverage", False, N)
        assert got == want, (widths[:3], len(widths), N)
        assert form(rg, "ends", False, N)[0] is False and form(rg, "ends", True, N)[0] is False
        for flag in ("0", "1"):
            monkeypatch.setenv("BAMSIGNALS_SCALED_SEGMENTED", flag)
            forced, res = form(rg, "coverage", False, N)
            assert forced == (flag == "1") and np.array_equal(res, own)
            assert form(rg, "ends", True, N)[0] == (flag == "1")
        seen.add(got)
    assert seen == {False, True}
    monkeypatch.delenv("BAMSIGNALS_SCALED_SEGMENTED")
    rg = deck([10_000] * 3)
    other = SummaryPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params("coverage", False), ())
    assert lib.bsig_plan_scaled_segmented(other._h) == 0 and lib.bsig_plan_scaled_segmented(None) == 0
    other.close()


# ---- seams -----------------------------------------------------------------------------------------------------------
def _n_with_edge(w, cell):
    """the smallest N >= 2 one of whose bins begins exactly on `cell` (bin j begins on ceil(j * w / N))"""
    for N in range(2, 2049):
        if cell in (-(-np.arange(1, N, dtype=np.int64) * w // N)).tolist():
            return N
    raise AssertionError("no such N")


@pytest.mark.parametrize("segmented", ["0", "1"])
@pytest.mark.parametrize("tile", [64, 0])
def test_seams(synth, tile, segmented, monkeypatch):
    """one-base reads on the last cell of a tile and the first of the next and on cells 0 and w - 1 (cells in range
    orientation: a '-' range's tiles are cut from its other end), and bins that begin on the seam, one cell before it and
    one cell after it"""
    ctx = synth[0]
    monkeypatch.setenv("BAMSIGNALS_SCALED_SEGMENTED", segmented)
    loc = 40_000
    step = tile or 2048
    w = 3 * step + 17
    Ns = [_n_with_edge(w, step + d) for d in (0, -1, 1)] + [_n_with_edge(w, 2 * step)]
    assert all(2 <= N < w // 3 for N in Ns) and len(set(Ns)) >= 3
    for strand in (1, -1):
        def g(x):
            return loc + x if strand > 0 else loc + w - 1 - x
        parts = []
        for k, x in enumerate((0, step - 1, step, 2 * step - 1, 2 * step, w - 1)):
            parts += [de.planted(3 + k, 0, g(x), read_len=1), de.planted(11 + k, 0, g(x), reverse=True, read_len=1)]
        for x in (7, step + 9, w - 30):
            parts += [de.planted(2, 0, g(x), read_len=1), de.planted(1, 0, g(x), reverse=True, read_len=1)]
        cols = de.merge_sorted(parts, 1)
        cols["ref_len"] = np.asarray([200_000], np.int64)
        reads = _upload(ctx, cols)
        try:
            rg = dict(rid=[0], loc=[loc], len=[w], strand=[strand])
            for signal, ss in (("coverage", False), ("ends", False), ("ends", True)):
                cells = de.cells(cols, rg, signal, ss)
                rows = se.rows_of(cells, rg, ss)
                # (the planting took: the cells on both sides of a seam differ, so a cell in the wrong bin shows)
                for r in range(rows[0].shape[0]):
                    assert rows[0][r][step - 1] > 0 and rows[0][r][step] > 0 and rows[0][r][step - 1] != rows[0][r][step]
                    assert rows[0][r][0] > 0 and rows[0][r][w - 1] > 0
                for N in Ns + sorted({1, min(w, 2048), 2048}):
                    for threads in (64, 256):
                        got, st, _ = _check(ctx, reads, cells, rg, signal, ss, N, tile_cells=tile, threads=threads)
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
            monkeypatch.setenv("BAMSIGNALS_SCALED_RUN_TILES", per)
        else:
            monkeypatch.delenv("BAMSIGNALS_SCALED_RUN_TILES")
        results[per], st, counts[per] = _check(ctx, reads, cells, rg, signal, ss, 100, **kw)
    assert np.array_equal(results["1"], results["1000000"]) and np.array_equal(results["1"], results[None])
    tiles = 204 + 2 * ((REF_LEN[1] + 2047) // 2048)
    assert st["n_items"] == tiles == counts["1"] and counts["1000000"] == 1 and 1 < counts[None] <= tiles
    got = results[None]
    assert not got[200:203].any()
    assert np.array_equal(got[204], got[3]) and np.array_equal(got[205], got[3]) and np.array_equal(got[206], got[77])
    # the whole reference on '-' and on '+': the bins mirrored (700,017 is no multiple of 100: the bins' edges differ)
    assert got[203].min() > 0 and got[203].sum() == got[208].sum() and not np.array_equal(got[203], got[208][::-1, ::-1])


# ---- bin arithmetic past 32 bits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["cov", "ends-ss"])
def test_bin_arithmetic_past_32_bits(synth, variant):
    """w = 2,200,000 and N = 2,048: c * N passes 2^32 from cell 2,097,152 (bin 1,952) on"""
    ctx, cols, reads, orc = synth
    signal, ss, kw = VARIANTS[variant]
    w, N = 2_200_000, 2048
    assert REF_LEN[0] == 2_000_000 and 2_097_152 * N == 2 ** 32 and 2_097_152 * N // w == 1952
    rg = dict(rid=[0, 0], loc=[-300, -300], len=[w, w], strand=[1, -1])
    cells = de.cells(orc, rg, signal, ss, **kw)
    want = sc.from_cells(cells, rg, ss, N)
    # '+': the cells past 2^32 / N lie behind the reference's end; '-': they are the reference's start, and full of reads
    assert not want[0, :, 1952:].any() and want[0, :, 1:1800].sum(axis=0).min() > 0
    assert want[1, :, 1952:2047].sum(axis=0).min() > 0 and not want[1, :, :180].any()
    got, st, _ = _check(ctx, reads, cells, rg, signal, ss, N, **kw)
    assert st["n_items"] == 2 * ((w + 2047) // 2048)
    # w >= 2^23, where the kernel's quotient is a comparison: the reference's reads in the top bins of a '-' range
    w = 9_000_000
    rg = dict(rid=[0], loc=[-300], len=[w], strand=[-1])
    cells = de.cells(orc, rg, signal, ss, **kw)
    want = sc.from_cells(cells, rg, ss, N)
    assert w >= 2 ** 23 and want[0, :, 1600:2047].sum(axis=0).min() > 0 and not want[0, :, :1590].any()
    _check(ctx, reads, cells, rg, signal, ss, N, runs=1, **kw)


# ---- 16-bit -> wide --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32_767, 32_768])
@pytest.mark.parametrize("beside", [False, True])
def test_coverage_piles_around_the_16_bit_ceiling(synth, n, beside):
    ctx = synth[0]
    cols, reads, rg = _pile(ctx, n, beside)
    rg = _with_neighbours(rg)
    try:
        cells = de.cells(cols, rg, "coverage", False)
        got, st, _ = _check(ctx, reads, cells, rg, "coverage", False, 16)
        assert (got[:, 0, :].max(axis=1) >= n).all()
        assert (st["heavy_tiles"] > 0) == (n + (3000 if beside else 0) > 32_767), st["heavy_tiles"]
        assert st["n_items"] == 2 + 1 + 3
    finally:
        reads.close()


@pytest.mark.parametrize("n", [65_535, 65_536])
@pytest.mark.parametrize("beside", [False, True])
def test_end_piles_around_and_past_16_bits(synth, n, beside):
    ctx = synth[0]
    for reverse in (False, True):
        cols, reads, rg = _pile(ctx, n, beside, reverse=reverse)
        rg = _with_neighbours(rg)
        try:
            for ss in (False, True):
                cells = de.cells(cols, rg, "ends", ss)
                got, st, _ = _check(ctx, reads, cells, rg, "ends", ss, 16, runs=1)
                assert (got.max(axis=(1, 2)) >= n).all()
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
            got, st, _ = _check(ctx, reads, cells, rg, signal, ss, 50, **kw)
            assert got.sum() > 0
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
        got, st, n_runs = _run(ctx, reads, dict(rid=[], loc=[], len=[], strand=[]), signal, ss, 5, **kw)
        assert got.shape == (0, S, 5) and st["n_items"] == 0 and n_runs == 0
        got, st, n_runs = _run(ctx, reads, dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1]), signal, ss, 5, **kw)
        assert got.tolist() == [[[0] * 5] * S] * 2 and n_runs == 0
        # wholly outside the reference (behind the reads that hang over its end), and over both of its ends
        rg = dict(rid=[0, 1, 1], loc=[-500, 705_017, -300], len=[400, 100, REF_LEN[1] + 900], strand=[1, -1, -1])
        got, _, _ = _check(ctx, reads, de.cells(orc, rg, signal, ss, **kw), rg, signal, ss, 5, **kw)
        assert not got[:2].any() and got[2].sum() > 0


def test_a_shuffled_deck_gives_the_shuffled_rows(synth):
    ctx, cols, reads, orc = synth
    rg = _cat(_ranges(50, 3000, seed=3, jitter=2900), dict(rid=[0, 1], loc=[70, 80], len=[0, 5000], strand=[1, -1]))
    perm = np.random.default_rng(8).permutation(len(rg["len"]))
    shuffled = {k: v[perm] for k, v in rg.items()}
    for signal, ss, kw in VARIANTS.values():
        a, _, _ = _check(ctx, reads, de.cells(orc, rg, signal, ss, **kw), rg, signal, ss, 30, **kw)
        b, _, _ = _run(ctx, reads, shuffled, signal, ss, 30, runs=1, **kw)
        assert np.array_equal(b, a[perm]) and len(np.unique(a.sum(axis=(1, 2)))) > 20


# ---- plans -----------------------------------------------------------------------------------------------------------
def test_stale_plan_and_wrong_run_calls(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, HistPlan, Plan, ScaledPlan, SummaryPlan, SumPlan, XcorrPlan, make_params
    ctx, cols, _, _ = synth
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        a = ([0], [10], [100], [1])
        prof = make_params(_lib.MODE_PROFILE)
        mp = ScaledPlan(ctx, reads, *a, _params("coverage", False), 5)
        me = ScaledPlan(ctx, reads, *a, _params("ends", True), 3)
        pp, sp, xp = Plan(ctx, reads, *a, prof), SumPlan(ctx, reads, *a, prof), XcorrPlan(ctx, reads, *a, prof, 20)
        fp = FragPlan(ctx, reads, *a, make_params(_lib.MODE_COUNT, tlen_filter=(0, 24), binsize=-1, requiredF=66), 1)
        hp = HistPlan(ctx, reads, *a, _params("coverage", False), 24)
        yp = SummaryPlan(ctx, reads, *a, _params("coverage", False), (1, 5))
        b32, b64 = np.zeros(400, np.int32), np.zeros(400, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        host, dev = "a scaled plan runs with bsig_plan_run_scaled_host", "a scaled plan runs with bsig_plan_run_scaled"
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
                (lib.bsig_plan_run_summary_host, me, p64, host),
                (lib.bsig_plan_run_summary, mp, p64, dev),
                (lib.bsig_plan_run_scaled_host, pp, p64, "not a scaled plan: bsig_plan_run_host runs it"),
                (lib.bsig_plan_run_scaled, pp, p64, "not a scaled plan: bsig_plan_run runs it"),
                (lib.bsig_plan_run_scaled_host, sp, p64, "not a scaled plan: bsig_plan_run_sum_host runs it"),
                (lib.bsig_plan_run_scaled, sp, p64, "not a scaled plan: bsig_plan_run_sum runs it"),
                (lib.bsig_plan_run_scaled_host, xp, p64, "not a scaled plan: bsig_plan_run_xcorr_host runs it"),
                (lib.bsig_plan_run_scaled, xp, p64, "not a scaled plan: bsig_plan_run_xcorr runs it"),
                (lib.bsig_plan_run_scaled_host, fp, p64, "not a scaled plan: bsig_plan_run_frag_host runs it"),
                (lib.bsig_plan_run_scaled, fp, p64, "not a scaled plan: bsig_plan_run_frag runs it"),
                (lib.bsig_plan_run_scaled_host, hp, p64, "not a scaled plan: bsig_plan_run_hist_host runs it"),
                (lib.bsig_plan_run_scaled, hp, p64, "not a scaled plan: bsig_plan_run_hist runs it"),
                (lib.bsig_plan_run_scaled_host, yp, p64, "not a scaled plan: bsig_plan_run_summary_host runs it"),
                (lib.bsig_plan_run_scaled, yp, p64, "not a scaled plan: bsig_plan_run_summary runs it")):
            assert fn(plan._h, buf) == -1
            assert lib.bsig_last_error().decode() == says
        assert not b32.any() and not b64.any()
        h = C.c_void_p()
        assert lib.bsig_plan_runs_create(mp._h, C.byref(h)) == -1
        assert lib.bsig_last_error().decode() == "a scaled plan has no per-range result to encode"
        for other in (pp, sp, xp, fp, hp, yp):
            assert lib.bsig_plan_scaled_cells(other._h) == 0 and lib.bsig_plan_scaled_runs(other._h) == 0
        assert lib.bsig_plan_scaled_cells(mp._h) == 5 and lib.bsig_plan_scaled_cells(me._h) == 6
        assert lib.bsig_plan_scaled_cells(None) == 0 and lib.bsig_plan_scaled_runs(None) == 0 and lib.bsig_plan_scaled_runs(mp._h) == 1
        assert lib.bsig_plan_hist_cells(mp._h) == 0 and lib.bsig_plan_sum_cells(mp._h) == 0 and lib.bsig_plan_frag_cells(mp._h) == 0
        assert lib.bsig_plan_summary_cells(mp._h) == 0 and lib.bsig_plan_summary_runs(me._h) == 0
        first = mp.run_host()
        assert first.shape == (1, 1, 5) and first.min() > 0 and first.sum() == yp.run_host()[0, 0, 0]
        assert np.array_equal(mp.run_host(), first) and np.array_equal(mp.run_host(), first)
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        with pytest.raises(_lib.BsigError, match="make a new plan"):
            mp.run_host()
        mp2 = ScaledPlan(ctx, reads, *a, _params("coverage", False), 5)
        assert np.array_equal(mp2.run_host(), first)
        for p in (mp, mp2, me, pp, sp, xp, fp, hp, yp):
            p.close()
    finally:
        reads.close()


def test_errors(synth):
    """the parameter rule's table (tests/test_scaled_cpu.py) and what only the plan call can express"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import ScaledPlan, make_params
    ctx, cols, reads, _ = synth
    a = ([0], [10], [100], [1])
    for kw, code, message in PARAM_RULE:
        tf = kw.get("tlen_filter", ())
        p = _lib.Params()
        p.mode, p.binsize, p.filteredF = (_lib.MODE_COVERAGE if kw["signal"] == "coverage" else _lib.MODE_PROFILE), 1, -1
        p.ss, p.tspan, p.pe_mid = kw.get("ss", 0), kw.get("tspan", 0), kw.get("pe_mid", 0)
        p.n_tlen_filter = len(tf)
        for i, v in enumerate(tf):
            p.tlen_filter[i] = v
        with pytest.raises(_lib.BsigError) as e:
            ScaledPlan(ctx, reads, *a, p, kw.get("n_bins", 10))
        assert (e.value.code, str(e.value)) == (code, message)
    for p, message in (
            (make_params(_lib.MODE_COUNT, binsize=-1), "the scaled regions bin per-base cells: bamCount has one cell per range"),
            (make_params(_lib.MODE_COVERAGE_EX), "the scaled regions of coverage are per base and unstranded: mode BSIG_MODE_COVERAGE"),
            (make_params(_lib.MODE_PROFILE, binsize=2), "the scaled regions cut per-base cells into n_bins bins: binsize must be 1"),
            (make_params(_lib.MODE_PROFILE, shift=1), "the scaled regions bin unshifted positions: shift must be 0"),
            (make_params(_lib.MODE_COVERAGE, shift=-1), "the scaled regions bin unshifted positions: shift must be 0"),
            (make_params(_lib.MODE_COVERAGE, ss=True), "the scaled regions of coverage have no strands: ss must be 0"),
            (make_params(_lib.MODE_PROFILE, threads=96), "threads must be 64, 128 or 256"),
            (make_params(_lib.MODE_COVERAGE, tile_cells=8), "tile_cells must be between 16 and 2048"),
            (make_params(_lib.MODE_PROFILE, tile_cells=2049), "tile_cells must be between 16 and 2048"),
            (make_params(7), "unknown mode 7")):
        with pytest.raises(_lib.BsigError) as e:
            ScaledPlan(ctx, reads, *a, p, 10)
        assert (e.value.code_name, str(e.value)) == ("BSIG_ERR_ARG", message)
    with pytest.raises(_lib.BsigError) as e:
        ScaledPlan(ctx, reads, [5], [10], [100], [1], _params("coverage", False), 10)
    assert e.value.code_name == "BSIG_ERR_CHROM"
    with pytest.raises(_lib.BsigError, match="negative width") as e:
        ScaledPlan(ctx, reads, [0], [10], [-1], [1], _params("ends", True), 10)
    assert e.value.code_name == "BSIG_ERR_ARG"
    # the edges of what is allowed
    for tile, N in ((16, 1), (2048, 2048)):
        ScaledPlan(ctx, reads, *a, _params("ends", True, tile_cells=tile), N).close()


# ---- file level ------------------------------------------------------------------------------------------------------
def test_file_level(fixture, decode_mode):
    from bamsignals_amd import ScaledSignals, bamCoverage, bamScaled, bamSummary
    gr, rg, cols, whole, whole_rg = fixture
    orc = de.oracle_reads(cols)
    for signal, choices in (("coverage", ("ignore", "extend")), ("ends", ("ignore", "filter", "midpoint"))):
        for pe in choices:
            for ss in ((False,) if signal == "coverage" else (True, False)):
                want = sc.expected(orc, rg, signal, ss, 10, **_pe_kw(signal, pe))
                sg = bamScaled(BAM, gr, nbins=10, signal=signal, ss=ss, paired_end=pe, verbose=False)
                assert isinstance(sg, ScaledSignals) and sg.nbins == 10 and sg.sums.dtype == np.int64
                assert sg.sums.shape == ((50, 2, 10) if ss else (50, 10)) and sg.cells.shape == (50, 10)
                assert np.array_equal(sg.sums, want if ss else want[:, 0, :]), (signal, pe, ss)
                assert np.array_equal(sg.width, rg["len"]) and sg.sums.sum() > 0
                assert np.array_equal(sg.cells, [sc.bin_sizes(w, 10) for w in rg["len"]])
                rs = bamSummary(BAM, gr, thresholds=(), signal=signal, ss=ss, paired_end=pe, verbose=False)
                assert np.array_equal(sg.sums.sum(axis=-1), rs.sum)
                one = bamScaled(BAM, gr, nbins=1, signal=signal, ss=ss, paired_end=pe, verbose=False)
                assert np.array_equal(one.sums[..., 0], rs.sum)
    # whole chromosomes in 2,048 bins
    sg = bamScaled(BAM, whole, nbins=2048, verbose=False)
    cov = bamCoverage(BAM, whole, verbose=False)
    assert sg.sums.sum(axis=1).tolist() == [int(np.asarray(s, np.int64).sum()) for s in cov] and (sg.sums.max(axis=1) > 0).all()
    # w / 5 bins are bins of 5 cells: bamCoverage's own
    fives = [i for i, w in enumerate(rg["len"].tolist()) if w % 5 == 0]
    assert len(fives) >= 3
    for i in fives:
        sg = bamScaled(BAM, gr[i], nbins=int(rg["len"][i]) // 5, mapqual=30, filteredFlag=1024, verbose=False)
        binned = bamCoverage(BAM, gr[i], mapqual=30, filteredFlag=1024, binsize=5, verbose=False)
        assert sg.sums[0].tolist() == np.asarray(binned[0], np.int64).reshape(-1).tolist()
        assert (sg.cells == 5).all()


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import _lib, bamScaled
    from bamsignals_amd.wrappers import last_call_route
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        for kw in (dict(signal="coverage", paired_end="extend"), dict(signal="ends", ss=True, paired_end="midpoint")):
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
            one = bamScaled(BAM, gr, nbins=33, verbose=False, **kw)
            assert "1 GPU slot(s)" in last_call_route() and "scaled" in last_call_route()
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
            four = bamScaled(BAM, gr, nbins=33, verbose=False, **kw)
            assert "4 GPU slot(s)" in last_call_route()
            assert "scaled of 4 blocks of ranges, rows placed on the host" in last_call_route()
            assert np.array_equal(one.sums, four.sums) and one.sums.any()
    finally:
        _lib.load().bsig_cache_clear()


# ---- the use ---------------------------------------------------------------------------------------------------------
def test_gene_bodies_of_unequal_width_pool_into_one_metaprofile(synth, tmp_path):
    """the synthetic background plus 30 "genes" of widths 500 .. 20,000 on both strands, each with a plateau of reads over
    its first tenth in transcript orientation: pooled over the genes, bin 0 of ten stands out on both strands"""
    from bamsignals_amd import GRanges, _lib, bamCoverage, bamScaled, write_columns_as_bam
    ctx, bg, _, _ = synth
    ref_off = np.asarray(bg["ref_off"])
    rng = np.random.default_rng(21)
    n = 30
    rid = np.arange(n) % 2
    width = np.exp(rng.uniform(np.log(500), np.log(20_000), n)).astype(np.int64)
    width[:2] = (500, 20_000)
    loc = 15_000 + 22_000 * np.arange(n)
    strand = np.where(np.arange(n) % 4 < 2, 1, -1)
    parts = [dict(rid=np.repeat(np.arange(2), np.diff(ref_off)), pos=bg["pos"], end=bg["end"], flag=bg["flag"], mapq=bg["mapq"],
                  tlen=bg["tlen"])]
    for i in range(n):
        tenth = int(width[i]) // 10
        first = loc[i] if strand[i] > 0 else loc[i] + width[i] - tenth          # the tenth at the gene's 5' end
        k = 10 * tenth                                                          # 400 reads deep
        parts.append(de.planted(k, 150, first + rng.integers(0, max(tenth - 40, 1), k), rid=rid[i]))
    cols = de.merge_sorted(parts, 2)
    cols["ref_len"] = np.asarray(REF_LEN, np.int64)
    bam = str(tmp_path / "genes.bam")
    cig = dict(cigar_off=np.arange(len(cols["pos"]) + 1, dtype=np.int64),
               cigar=((cols["end"].astype(np.int64) - cols["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(bam, ["chrA", "chrB"], dict(cols, **cig))
    try:
        gr = GRanges([("chrA", "chrB")[r] for r in rid], loc + 1, width=width, strand=["+" if s > 0 else "-" for s in strand])
        sg = bamScaled(bam, gr, nbins=10, verbose=False)
        for sel in (strand > 0, strand < 0):
            s, c = sg.sums[sel].sum(axis=0), sg.cells[sel].sum(axis=0)
            mean = s / c
            assert int(np.argmax(mean)) == 0 and mean[0] > 5 * mean[1:].max(), mean
        s, c = sg.pooled()
        assert int(np.argmax(s / c)) == 0 and int(c.sum()) == int(width.sum())
        # the matrix, row for row, from the per-base cells
        per_base = bamCoverage(bam, gr, verbose=False)
        m = sg.matrix()
        for i in range(n):
            cells = np.asarray(per_base[i], np.int64)
            edges = -(-np.arange(10, dtype=np.int64) * int(width[i]) // 10)
            assert np.array_equal(np.add.reduceat(cells, edges), sg.sums[i])
            assert np.array_equal(m[i], np.add.reduceat(cells, edges) / sg.cells[i])
    finally:
        _lib.load().bsig_cache_clear()
