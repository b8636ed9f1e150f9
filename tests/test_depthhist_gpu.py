"""GPU: the depth histogram over ranges (bsig_plan_create_hist, k_hist_tiles; bamDepthHist) against the definition --
np.bincount of the C oracle's per-base cells, then [cells, sum] (tests/depthhist_expected.py).  All exact.

The refusals for a run past 2^32 - 1 cells (the plan cuts its runs before that) and for a sum moment past 2^63 are not
exercised: no input a test can hold reaches them."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN

import depthhist_expected as de
from test_depthhist_cpu import PARAM_RULE

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [2_000_000, 700_017]
VS = (1, 7, 100, 8191)
# (name, signal, ss, the plan's parameters = the oracle's)
VARIANTS = {
    "cov": ("coverage", False, dict()),
    "cov-extend": ("coverage", False, dict(tspan=True, tlen_filter=(0, 1000), requiredF=66)),
    "ends": ("ends", False, dict()),
    "ends-ss": ("ends", True, dict()),
}
MORE = {
    "ends-ss-midpoint": ("ends", True, dict(pe_mid=True, tlen_filter=(0, 1000), requiredF=66)),
    "ends-filter-mapq": ("ends", False, dict(tlen_filter=(100, 400), requiredF=66, mapqual=30, filteredF=1024)),
    "cov-mapq": ("coverage", False, dict(mapqual=30, filteredF=1024)),
}


def _upload(ctx, cols):
    from bamsignals_amd.device import Reads
    if "cigar" in cols:
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                     cigar_off=cols["cigar_off"], cigar=cols["cigar"])
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])


@pytest.fixture(scope="module")
def synth():
    """paired reads on two references, resident on GPU 0, and the oracle's copy of them"""
    from bamsignals_amd.device import Context
    from bamsignals_amd.synth import synth_reads
    from oracle import oracle_c
    ctx = Context(0)
    cols = synth_reads(400_000, REF_LEN, seed=92, paired=True)
    cols["end"] = oracle_c.cigar_end(cols["pos"], cols["flag"], cols["cigar_off"], cols["cigar"])
    reads = _upload(ctx, cols)
    yield ctx, cols, reads, de.oracle_reads(cols)
    reads.close()
    ctx.close()


def _params(signal, ss, **kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    if signal == "coverage":
        return make_params(_lib.MODE_COVERAGE, ss=ss, **kw)
    return make_params(_lib.MODE_PROFILE, binsize=1, ss=ss, **kw)


def _run(ctx, reads, rg, signal, ss, V, runs=2, **kw):
    """a plan's first run (fused lookups) and its later ones (windows kept), which must agree; (result, stats, runs)"""
    from bamsignals_amd.device import HistPlan
    plan = HistPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(signal, ss, **kw), V)
    try:
        assert plan.cells == V + 3
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int64 and got[0].shape == (plan.cells,)
        return got[0], plan.stats(), plan.runs
    finally:
        plan.close()


def _oracle_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("tile_cells", "threads")}


def _diff(got, want):
    return np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8]


def _check(ctx, reads, cells, rg, signal, ss, V, runs=2, **kw):
    """cells: the oracle's cells of these ranges and parameters (computed once, shared among the max_values)"""
    got, st, n_runs = _run(ctx, reads, rg, signal, ss, V, runs=runs, **kw)
    want = de.from_cells(cells, V)
    assert np.array_equal(got, want), (signal, ss, V, kw, _diff(got, want))
    assert st["cells"] == V + 3
    return got, st, n_runs


def _ranges(n, w, seed, jitter=0):
    from bamsignals_amd.synth import synth_ranges
    return synth_ranges(n, w, REF_LEN, seed=seed, jitter=jitter)


def _cat(*rgs):
    return {k: np.concatenate([np.asarray(r[k], np.int32) for r in rgs]) for k in ("rid", "loc", "len", "strand")}


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("w", [1, 100, 2048, 2049, 10_000])
def test_grid(synth, w, variant):
    ctx, cols, reads, orc = synth
    signal, ss, kw = VARIANTS[variant]
    rg = _ranges(60 if w < 10_000 else 12, w, seed=w)
    assert w >= 10_000 or len(set(rg["strand"].tolist())) == 3
    cells = de.cells(orc, rg, signal, ss, **kw)
    # (not vacuous, on the expected side first: the overflow row is in use for some max_value and empty for another)
    over = [int(de.from_cells(cells, V)[V]) for V in VS]
    assert max(over) > 0 and min(over) == 0, over
    for V in VS:
        got, st, _ = _check(ctx, reads, cells, rg, signal, ss, V, **kw)
        assert st["heavy_tiles"] == 0
        if w >= 2048 and V >= 7:
            assert np.count_nonzero(got[:V + 1]) >= 3
        assert got[V + 1] == de.n_cells(rg, ss) == got[:V + 1].sum()


@pytest.mark.parametrize("variant", sorted(MORE))
def test_filters_and_the_midpoint_rule(synth, variant):
    ctx, cols, reads, orc = synth
    signal, ss, kw = MORE[variant]
    rg = _ranges(40, 3000, seed=5, jitter=800)
    cells = de.cells(orc, rg, signal, ss, **kw)
    assert cells.sum() > 1000
    for V in (3, 100):
        _check(ctx, reads, cells, rg, signal, ss, V, **kw)


def test_stats_are_the_ordinary_plans(synth):
    from bamsignals_amd.device import Plan
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 5000, seed=2048)
    for signal, ss, kw in list(VARIANTS.values()) + list(MORE.values()):
        for tile in (2048, 512):
            got, st, _ = _run(ctx, reads, rg, signal, ss, 100, runs=1, tile_cells=tile, **kw)
            plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(signal, ss, tile_cells=tile, **kw))
            cs = plan.stats()
            plan.close()
            assert st["cells"] == 103 and st["heavy_tiles"] == 0 and st["n_ranges"] == 60
            assert st["n_items"] == cs["n_items"] == 60 * ((5000 + tile - 1) // tile)
            for k in ("visits", "visits_packed", "visits_short", "bytes_per_visit_packed", "bytes_per_visit_short",
                      "bytes_per_visit_long"):
                assert st[k] == cs[k], (signal, ss, kw, k)
            assert st["visits"] > 0
    # the default tile is 2,048 cells
    _, st, _ = _run(ctx, reads, rg, "ends", True, 100, runs=1)
    assert st["n_items"] == 60 * 3


# ---- seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,w", [(64, 64 * 3 + 17), (0, 2048 * 2 + 100)])
def test_seams(synth, tile, w):
    """reads whose coverage steps and 5' ends fall on the first and last cell of the range and of each tile, and one base
    outside, on both strands; the range on either strand (a '-' range's tiles are cut from its other end)"""
    ctx = synth[0]
    loc = 40_000
    step = tile or 2048
    xs = [-1, 0, step - 1, step, 2 * step - 1, 2 * step, w - 1, w]
    xs = sorted(set(xs + [w - 1 - x for x in xs]))
    parts = []
    for k, x in enumerate(xs):
        t = loc + x
        parts.append(de.planted(1 + k % 3, 0, t))                        # forward: begins to cover on t, 5' end on t
        parts.append(de.planted(1 + (k + 1) % 3, 0, t, reverse=True))    # reverse: covers up to t, 5' end on t
        parts.append(de.planted(1, 0, t - 39))                           # forward: covers up to t
        parts.append(de.planted(2, 0, t + 39, reverse=True))             # reverse: begins to cover on t
    cols = de.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        for strand in (1, -1):
            rg = dict(rid=[0], loc=[loc], len=[w], strand=[strand])
            for signal, ss in (("coverage", False), ("ends", False), ("ends", True)):
                cells = de.cells(cols, rg, signal, ss)
                assert np.count_nonzero(np.bincount(cells)) >= 4          # (the planting took: several depths)
                for threads in (64, 256):
                    got, st, _ = _check(ctx, reads, cells, rg, signal, ss, 5, tile_cells=tile, threads=threads)
                    assert st["n_items"] == (w + step - 1) // step and st["heavy_tiles"] == 0
    finally:
        reads.close()


# ---- the overflow row's edge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [7, 100])
def test_overflow_rows_edge(synth, V):
    """piles of exactly V - 1, V and V + 1 reads on one base"""
    ctx = synth[0]
    parts = [de.planted(V - 1, 0, 50_000), de.planted(V, 0, 50_500), de.planted(V + 1, 0, 51_000),
             de.planted(V - 1, 0, 52_000, reverse=True), de.planted(V + 1, 0, 52_500, reverse=True)]
    cols = de.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=[0, 0], loc=[49_000, 50_400], len=[5000, 300], strand=[1, -1])
        for signal, ss in (("coverage", False), ("ends", False), ("ends", True)):
            cells = de.cells(cols, rg, signal, ss)
            per = 40 if signal == "coverage" else 1
            want = de.from_cells(cells, V)
            # piles of V - 1: two; of V: one, seen by both ranges; of V + 1: two
            assert want[V - 1] == 2 * per and want[V] == 4 * per and want[V + 2] == per * (2 * (V - 1) + 2 * V + 2 * (V + 1))
            got, _, _ = _check(ctx, reads, cells, rg, signal, ss, V)
            assert (got[V - 1], got[V]) == (want[V - 1], want[V])
    finally:
        reads.close()


# ---- 16-bit -> wide --------------------------------------------------------------------------------------------------
def _pile(ctx, n, beside, reverse=False):
    parts = [de.planted(n, 0, 50_000, reverse=reverse)]
    if beside:
        rng = np.random.default_rng(n)
        p = rng.integers(49_100, 50_900, 3000)
        parts.append(dict(rid=np.zeros(3000, np.int64), pos=p, end=p + 49, flag=np.where(rng.random(3000) < 0.5, 0, 16),
                          mapq=np.full(3000, 30)))
    cols = de.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    return cols, _upload(ctx, cols), dict(rid=[0, 0], loc=[49_000, 49_990], len=[3000, 20], strand=[1, -1])


@pytest.mark.parametrize("n", [32_766, 32_767, 32_768, 32_769])
@pytest.mark.parametrize("beside", [False, True])
def test_coverage_piles_around_the_16_bit_ceiling(synth, n, beside, monkeypatch):
    """a signed 16-bit difference cell may see 32,767 reads: one more in the tile's windows and the tile takes the int32
    image.  With max_value = 8,191 the pile lands in the overflow row and the sum moment carries its true height."""
    ctx = synth[0]
    cols, reads, rg = _pile(ctx, n, beside)
    try:
        cells = de.cells(cols, rg, "coverage", False)
        assert cells.max() >= n and de.from_cells(cells, 8191)[8191] >= 40 + 10
        for form in ("plain", "merge"):
            monkeypatch.setenv("BAMSIGNALS_HIST_FORM", form)
            got, st, _ = _check(ctx, reads, cells, rg, "coverage", False, 8191)
            assert got[8193] >= 50 * n
            assert (st["heavy_tiles"] > 0) == (n + (3000 if beside else 0) > 32_767), st["heavy_tiles"]
    finally:
        reads.close()


@pytest.mark.parametrize("n", [32_768, 32_769, 65_535, 65_536, 65_537])
@pytest.mark.parametrize("beside", [False, True])
def test_end_piles_around_and_past_16_bits(synth, n, beside, monkeypatch):
    """an unsigned 16-bit cell may see 32,768 reads; piles past 65,535 would wrap one"""
    ctx = synth[0]
    for reverse in (False, True):
        cols, reads, rg = _pile(ctx, n, beside, reverse=reverse)
        try:
            for ss in (False, True):
                cells = de.cells(cols, rg, "ends", ss)
                assert cells.max() >= n
                for form in ("plain", "merge"):
                    monkeypatch.setenv("BAMSIGNALS_HIST_FORM", form)
                    got, st, _ = _check(ctx, reads, cells, rg, "ends", ss, 8191, runs=1)
                    assert got[8191] >= 2 and got[8193] >= 2 * n
                    assert (st["heavy_tiles"] > 0) == (n + (3000 if beside else 0) > 32_768), st["heavy_tiles"]
        finally:
            reads.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_lowered_ceiling_runs_the_grid_wide(synth, variant, monkeypatch):
    ctx, cols, reads, orc = synth
    signal, ss, kw = VARIANTS[variant]
    rg = _ranges(60, 2048, seed=2048)
    cells = de.cells(orc, rg, signal, ss, **kw)
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    for form in ("plain", "merge"):
        monkeypatch.setenv("BAMSIGNALS_HIST_FORM", form)
        for V in (7, 100):
            got, st, n_runs = _check(ctx, reads, cells, rg, signal, ss, V, **kw)
            assert st["heavy_tiles"] >= 50 and np.count_nonzero(got[:V + 1]) >= 3
            assert n_runs >= st["heavy_tiles"]


# ---- forms, threads, runs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "merge"])
def test_forms_and_threads(synth, form, monkeypatch):
    ctx, cols, reads, orc = synth
    monkeypatch.setenv("BAMSIGNALS_HIST_FORM", form)
    rg = _ranges(40, 3000, seed=5, jitter=800)
    for signal, ss, kw in list(VARIANTS.values()) + [MORE["ends-ss-midpoint"]]:
        cells = de.cells(orc, rg, signal, ss, **kw)
        for threads in (64, 128, 256):
            _check(ctx, reads, cells, rg, signal, ss, 9, threads=threads, **kw)


def test_run_lengths_and_the_lowered_ceiling(synth, monkeypatch):
    """one tile per workgroup, all tiles in one, and runs cut by the cells of their tiles"""
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 2048, seed=2048)
    for signal, ss, kw in VARIANTS.values():
        cells = de.cells(orc, rg, signal, ss, **kw)
        for form in ("merge", "plain"):
            monkeypatch.setenv("BAMSIGNALS_HIST_FORM", form)
            counts = {}
            for per in ("1", "1000000", None):
                if per:
                    monkeypatch.setenv("BAMSIGNALS_HIST_RUN_TILES", per)
                else:
                    monkeypatch.delenv("BAMSIGNALS_HIST_RUN_TILES")
                _, st, counts[per] = _check(ctx, reads, cells, rg, signal, ss, 100, **kw)
            assert counts["1"] == st["n_items"] == 60 and counts["1000000"] == 1 and 1 <= counts[None] <= 60
            # 60 tiles of 2,048 cells (4,096 with strands): a ceiling of 5,000 cells ends a run after two tiles (one)
            monkeypatch.setenv("BAMSIGNALS_HIST_RUN_TILES", "1000000")
            monkeypatch.setenv("BAMSIGNALS_HIST_FLUSH_CELLS", "5000")
            _, st, cut = _check(ctx, reads, cells, rg, signal, ss, 100, **kw)
            assert 60 >= cut >= 20 and cut == (60 if ss else 30)
            monkeypatch.delenv("BAMSIGNALS_HIST_FLUSH_CELLS")
            monkeypatch.delenv("BAMSIGNALS_HIST_RUN_TILES")


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
            assert got[52] > 0
            if env.get("BAMSIGNALS_PACK") == "0":
                assert st["visits_packed"] == 0
            else:
                half = signal == "ends" and not kw and not env
                assert st["visits_packed"] > 0 and st["bytes_per_visit_packed"] == (2 if half else 8 if "tlen_filter" in kw else 4)
    finally:
        reads.close()


# ---- whole references, odd ranges and the moments --------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["cov", "ends", "ends-ss"])
def test_whole_references_odd_ranges_and_the_moments(synth, variant):
    """both references whole, short ranges, zero widths, duplicates, overhangs on both ends: one call; the strand of a
    range does not matter"""
    from oracle import oracle_c
    ctx, cols, reads, orc = synth
    signal, ss, kw = VARIANTS[variant]
    whole = dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[1, -1])
    short = _ranges(40, 300, seed=8, jitter=290)
    edge = dict(rid=[0, 0, 1, 1, 0, 0, 1], loc=[-700, 1_999_500, -3, 700_000, 5000, 5000, 40], len=[1500, 900, 10, 600, 0, 777, 0],
                strand=[1, -1, 0, 1, 1, -1, 0])
    rg = _cat(whole, short, edge, short, dict(rid=[0, 0], loc=[5000, 5000], len=[777, 777], strand=[-1, -1]))
    cells = de.cells(orc, rg, signal, ss, **kw)
    V = 40
    got, _, _ = _check(ctx, reads, cells, rg, signal, ss, V, **kw)
    assert got[V + 1] == de.n_cells(rg, ss) == got[:V + 1].sum()
    if signal == "coverage":
        assert got[V + 2] == int(cells.sum()) > 30_000_000
    else:
        counted, _ = oracle_c.pileup_core(orc, rg, binsize=-1, shift=0, ss=False, **kw)
        assert got[V + 2] == int(np.asarray(counted, np.int64).sum()) > 390_000
    flipped = dict(rg, strand=-np.asarray(rg["strand"]))
    for strands in (flipped, dict(rg, strand=np.zeros_like(rg["strand"]))):
        assert np.array_equal(_run(ctx, reads, strands, signal, ss, V, runs=1, **kw)[0], got)


def test_edges(synth):
    ctx, cols, reads, orc = synth
    for signal, ss, kw in VARIANTS.values():
        got, st, n_runs = _run(ctx, reads, dict(rid=[], loc=[], len=[], strand=[]), signal, ss, 500, **kw)
        assert got.shape == (503,) and not got.any() and st["n_items"] == 0 and n_runs == 0
        got, st, n_runs = _run(ctx, reads, dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1]), signal, ss, 7, **kw)
        assert got.shape == (10,) and not got.any() and n_runs == 0
    # ranges wholly outside their reference: cells of value 0 (the synthetic reads hang over their reference's end by a
    # few hundred bases, so "outside" begins behind those)
    rg = dict(rid=[0, 1], loc=[-500, 705_017], len=[400, 100], strand=[1, -1])
    assert de.expected(orc, rg, "ends", True, 3).tolist() == [1000, 0, 0, 0, 1000, 0]
    got, _, _ = _run(ctx, reads, rg, "ends", True, 3)
    assert got.tolist() == [1000, 0, 0, 0, 1000, 0]
    rg = dict(rid=[0, 1], loc=[-500, 700_017], len=[400, 100], strand=[1, -1])
    for signal, ss in (("ends", True), ("coverage", False)):
        _check(ctx, reads, de.cells(orc, rg, signal, ss), rg, signal, ss, 3)


# ---- plans -----------------------------------------------------------------------------------------------------------
def test_stale_plan_and_wrong_run_calls(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, HistPlan, Plan, SumPlan, XcorrPlan, make_params
    ctx, cols, _, _ = synth
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        a = ([0], [10], [100], [1])
        prof = make_params(_lib.MODE_PROFILE)
        hp = HistPlan(ctx, reads, *a, _params("coverage", False), 24)
        he = HistPlan(ctx, reads, *a, _params("ends", True), 5)
        pp, sp, xp = Plan(ctx, reads, *a, prof), SumPlan(ctx, reads, *a, prof), XcorrPlan(ctx, reads, *a, prof, 20)
        fp = FragPlan(ctx, reads, *a, make_params(_lib.MODE_COUNT, tlen_filter=(0, 24), binsize=-1, requiredF=66), 1)
        b32, b64 = np.zeros(400, np.int32), np.zeros(400, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        host, dev = "a hist plan runs with bsig_plan_run_hist_host", "a hist plan runs with bsig_plan_run_hist"
        for fn, plan, buf, says in (
                (lib.bsig_plan_run_host, hp, p32, host),
                (lib.bsig_plan_run, hp, p32, dev),
                (lib.bsig_plan_run_host_async, hp, p32, dev),
                (lib.bsig_plan_run_sum_host, hp, p64, host),
                (lib.bsig_plan_run_sum, hp, p64, dev),
                (lib.bsig_plan_run_xcorr_host, hp, p64, host),
                (lib.bsig_plan_run_xcorr, hp, p64, dev),
                (lib.bsig_plan_run_frag_host, he, p64, host),
                (lib.bsig_plan_run_frag, he, p64, dev),
                (lib.bsig_plan_run_hist_host, pp, p64, "not a hist plan: bsig_plan_run_host runs it"),
                (lib.bsig_plan_run_hist, pp, p64, "not a hist plan: bsig_plan_run runs it"),
                (lib.bsig_plan_run_hist_host, sp, p64, "not a hist plan: bsig_plan_run_sum_host runs it"),
                (lib.bsig_plan_run_hist, sp, p64, "not a hist plan: bsig_plan_run_sum runs it"),
                (lib.bsig_plan_run_hist_host, xp, p64, "not a hist plan: bsig_plan_run_xcorr_host runs it"),
                (lib.bsig_plan_run_hist, xp, p64, "not a hist plan: bsig_plan_run_xcorr runs it"),
                (lib.bsig_plan_run_hist_host, fp, p64, "not a hist plan: bsig_plan_run_frag_host runs it"),
                (lib.bsig_plan_run_hist, fp, p64, "not a hist plan: bsig_plan_run_frag runs it"),
                # (the refusals that were there keep their words)
                (lib.bsig_plan_run_frag_host, pp, p64, "not a frag plan: bsig_plan_run_host runs it"),
                (lib.bsig_plan_run_host, fp, p32, "a frag plan runs with bsig_plan_run_frag_host")):
            assert fn(plan._h, buf) == -1
            assert lib.bsig_last_error().decode() == says
        assert not b32.any() and not b64.any()
        h = C.c_void_p()
        assert lib.bsig_plan_runs_create(hp._h, C.byref(h)) == -1
        assert lib.bsig_last_error().decode() == "a hist plan has no per-range result to encode"
        for other in (pp, sp, xp, fp):
            assert lib.bsig_plan_hist_cells(other._h) == 0 and lib.bsig_plan_hist_runs(other._h) == 0
        assert lib.bsig_plan_hist_cells(hp._h) == 27 and lib.bsig_plan_hist_cells(None) == 0 and lib.bsig_plan_hist_runs(hp._h) == 1
        assert lib.bsig_plan_xcorr_cells(hp._h) == 0 and lib.bsig_plan_sum_cells(hp._h) == 0 and lib.bsig_plan_frag_cells(hp._h) == 0
        first = hp.run_host()
        assert first[25] == 100 and first[:25].sum() == 100
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        with pytest.raises(_lib.BsigError, match="make a new plan"):
            hp.run_host()
        hp2 = HistPlan(ctx, reads, *a, _params("coverage", False), 24)
        assert np.array_equal(hp2.run_host(), first)
        for p in (hp, hp2, he, pp, sp, xp, fp):
            p.close()
    finally:
        reads.close()


def test_errors(synth):
    """the parameter rule's table (tests/test_depthhist_cpu.py) and what only the plan call can express"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import HistPlan
    ctx, cols, reads, _ = synth
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
        with pytest.raises(_lib.BsigError) as e:
            HistPlan(ctx, reads, *a, p, kw.get("max_value", 100))
        assert (e.value.code, str(e.value)) == (code, message)

    def params(mode, **kw):
        from bamsignals_amd.device import make_params
        return make_params(mode, **kw)
    for p, message in (
            (params(_lib.MODE_COUNT, binsize=-1), "the depth histogram counts per-base cells: bamCount has one cell per range"),
            (params(_lib.MODE_COVERAGE_EX), "the depth histogram of coverage is per base and unstranded: mode BSIG_MODE_COVERAGE"),
            (params(_lib.MODE_PROFILE, binsize=2), "the depth histogram is per base: binsize must be 1"),
            (params(_lib.MODE_PROFILE, shift=1), "the depth histogram counts unshifted positions: shift must be 0"),
            (params(_lib.MODE_COVERAGE, shift=-1), "the depth histogram counts unshifted positions: shift must be 0"),
            (params(_lib.MODE_COVERAGE, ss=True), "the depth histogram of coverage has no strands: ss must be 0"),
            (params(_lib.MODE_PROFILE, threads=96), "threads must be 64, 128 or 256"),
            (params(_lib.MODE_COVERAGE, tile_cells=8), "tile_cells must be between 16 and 2048"),
            (params(_lib.MODE_PROFILE, tile_cells=2049), "tile_cells must be between 16 and 2048"),
            (params(7), "unknown mode 7")):
        with pytest.raises(_lib.BsigError) as e:
            HistPlan(ctx, reads, *a, p, 100)
        assert (e.value.code_name, str(e.value)) == ("BSIG_ERR_ARG", message)
    with pytest.raises(_lib.BsigError) as e:
        HistPlan(ctx, reads, [5], [10], [100], [1], _params("coverage", False), 100)
    assert e.value.code_name == "BSIG_ERR_CHROM"
    with pytest.raises(_lib.BsigError, match="negative width") as e:
        HistPlan(ctx, reads, [0], [10], [-1], [1], _params("ends", True), 100)
    assert e.value.code_name == "BSIG_ERR_ARG"
    # the edges of what is allowed
    for tile, V in ((16, 1), (2048, 8191)):
        HistPlan(ctx, reads, *a, _params("ends", True, tile_cells=tile), V).close()


# ---- file level ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(fixture_reads):
    from bamsignals_amd import GRanges
    fx = fixture_reads
    names = [str(s) for s in fx["ref_names"]]
    rng = np.random.default_rng(29)
    n = 50
    rid = rng.integers(0, len(names), n).astype(np.int32)
    w = rng.integers(1, 4000, n).astype(np.int32)
    loc = np.asarray([rng.integers(0, int(fx["ref_len"][r]) - 100) for r in rid], np.int32)
    strand = np.asarray([1, -1, 0], np.int32)[rng.integers(0, 3, n)]
    gr = GRanges([names[r] for r in rid], loc + 1, width=w, strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in strand])
    rg = dict(rid=rid, loc=loc, len=w, strand=strand)
    cols = dict(ref_off=fx["ref_off"], pos=fx["bam_pos"], end=fx["bam_end"], flag=fx["bam_flag"], mapq=fx["bam_mapq"],
                tlen=fx["bam_tlen"])
    whole = GRanges(names[:3], [1, 1, 1], width=[int(x) for x in fx["ref_len"][:3]], strand=["+", "-", "*"])
    whole_rg = dict(rid=[0, 1, 2], loc=[0, 0, 0], len=[int(x) for x in fx["ref_len"][:3]], strand=[1, -1, 0])
    return gr, rg, cols, whole, whole_rg


@pytest.fixture(params=["all", "regions"])
def decode_mode(request, monkeypatch):
    from bamsignals_amd import _lib
    monkeypatch.setenv("BAMSIGNALS_DECODE", request.param)
    _lib.load().bsig_cache_clear()
    yield request.param
    _lib.load().bsig_cache_clear()


def _pe_kw(signal, pe):
    if pe == "ignore":
        return dict()
    kw = dict(requiredF=66, tlen_filter=(0, 1000))
    if pe == "extend":
        kw["tspan"] = True
    if pe == "midpoint":
        kw["pe_mid"] = True
    return kw


def test_the_fixture_is_what_the_issue_says(fixture):
    gr, rg, cols, whole, whole_rg = fixture
    for r, (cov, ends) in enumerate(((208, 11), (184, 9), (199, 10))):
        one = {k: [v[r]] for k, v in whole_rg.items()}
        assert int(de.cells(cols, one, "coverage", False).max()) == cov
        assert int(de.cells(cols, one, "ends", True).max()) == ends


def test_file_level(fixture, decode_mode):
    from bamsignals_amd import DepthHist, bamCoverage, bamDepthHist
    gr, rg, cols, whole, whole_rg = fixture
    orc = de.oracle_reads(cols)
    for signal, choices in (("coverage", ("ignore", "extend")), ("ends", ("ignore", "filter", "midpoint"))):
        for pe in choices:
            for ss in ((False,) if signal == "coverage" else (True, False)):
                cells = de.cells(orc, rg, signal, ss, **_pe_kw(signal, pe))
                for V in (3, 1000):
                    dh = bamDepthHist(BAM, gr, maxdepth=V, signal=signal, ss=ss, paired_end=pe, verbose=False)
                    want = de.from_cells(cells, V)
                    assert isinstance(dh, DepthHist) and dh.counts.dtype == np.int64 and dh.maxdepth == V
                    assert np.array_equal(dh.counts, want[:V + 1]), (signal, pe, ss, V)
                    assert (dh.n, dh.total) == (int(want[V + 1]), int(want[V + 2])) and dh.total > 0
                    assert dh.n == int(np.sum(rg["len"])) * (2 if ss else 1)
    dh = bamDepthHist(BAM, gr, maxdepth=50, mapqual=30, filteredFlag=1024, verbose=False)
    assert np.array_equal(dh.counts, de.expected(orc, rg, "coverage", False, 50, mapqual=30, filteredF=1024)[:51])
    assert dh.total == int(np.sum(np.concatenate([np.asarray(s, np.int64) for s in
                                                  bamCoverage(BAM, gr, mapqual=30, filteredFlag=1024, verbose=False)])))
    # whole chromosomes: the per-base coverage peaks at 208 / 184 / 199, the per-strand 5'-end piles at 11 / 9 / 10
    cells = de.cells(orc, whole_rg, "coverage", False)
    for V, saturated in ((100, True), (255, False)):
        dh = bamDepthHist(BAM, whole, maxdepth=V, verbose=False)
        assert dh.saturated is saturated and np.array_equal(dh.counts, de.from_cells(cells, V)[:V + 1])
        assert dh.total == int(cells.sum()) and dh.n == sum(whole_rg["len"]) and dh.mean() == Fraction(int(cells.sum()), dh.n)
    for V, saturated in ((11, True), (12, False)):
        assert bamDepthHist(BAM, whole, maxdepth=V, signal="ends", verbose=False).saturated is saturated


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import bamDepthHist
    from bamsignals_amd.wrappers import last_call_route
    from bamsignals_amd import _lib
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        for kw in (dict(signal="coverage", paired_end="extend"), dict(signal="ends", paired_end="midpoint")):
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
            one = bamDepthHist(BAM, gr, maxdepth=30, verbose=False, **kw)
            assert "1 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
            four = bamDepthHist(BAM, gr, maxdepth=30, verbose=False, **kw)
            assert "4 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
            assert np.array_equal(one.counts, four.counts) and one.counts[1:].any()
            assert (one.n, one.total) == (four.n, four.total) and one.total > 0
    finally:
        _lib.load().bsig_cache_clear()


# ---- the use ---------------------------------------------------------------------------------------------------------
def test_duplication_and_breadth_are_read_off_the_data(synth, tmp_path):
    """the synthetic background plus 20,000 reads planted as exact duplicates, in groups of 4 at 5,000 sites where the
    background has no 5' end on that strand"""
    from bamsignals_amd import GRanges, bamDepthHist, write_columns_as_bam
    from bamsignals_amd import _lib
    ctx, bg, _, orc_bg = synth
    ref_off = np.asarray(bg["ref_off"])
    rg = dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[1, 0])
    bg_cells = de.cells(orc_bg, rg, "ends", True).reshape(-1, 2)[:REF_LEN[0], 0]       # reference 0, '+' range: sense = forward
    free = np.flatnonzero(bg_cells[:REF_LEN[0] - 1000] == 0)
    at = np.random.default_rng(4).choice(free, 5000, replace=False)
    parts = [dict(rid=np.repeat(np.arange(2), np.diff(ref_off)), pos=bg["pos"], end=bg["end"], flag=bg["flag"], mapq=bg["mapq"],
                  tlen=bg["tlen"]),
             de.planted(20_000, 150, np.repeat(at, 4))]
    cols = de.merge_sorted(parts, 2)
    cols["ref_len"] = np.asarray(REF_LEN, np.int64)
    V = 50
    before, want = de.expected(orc_bg, rg, "ends", True, V), de.expected(cols, rg, "ends", True, V)
    assert want[4] == before[4] + 5000 and want[V + 2] == before[V + 2] + 20_000 and want[V] == 0
    cov = de.cells(cols, rg, "coverage", False)
    bam = str(tmp_path / "dup.bam")
    cig = dict(cigar_off=np.arange(len(cols["pos"]) + 1, dtype=np.int64),
               cigar=((cols["end"].astype(np.int64) - cols["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(bam, ["chrA", "chrB"], dict(cols, **cig))
    try:
        gr = GRanges(["chrA", "chrB"], [1, 1], width=REF_LEN, strand=["+", "*"])
        dh = bamDepthHist(bam, gr, maxdepth=V, signal="ends", verbose=False)
        assert np.array_equal(dh.counts, want[:V + 1]) and not dh.saturated
        assert dh.counts[4] == before[4] + 5000
        assert dh.duplicate_fraction() == 1 - Fraction(int(np.count_nonzero(de.cells(cols, rg, "ends", True))), int(want[V + 2]))
        assert dh.duplicate_fraction() > Fraction(15_000, 420_000)
        dc = bamDepthHist(bam, gr, maxdepth=V, verbose=False)
        assert dc.breadth(1) == Fraction(int(np.count_nonzero(cov)), cov.size)
        assert dc.mean() == Fraction(int(cov.sum()), cov.size)
    finally:
        _lib.load().bsig_cache_clear()
