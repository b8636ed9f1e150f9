"""GPU: keepDup -- the capped plans (bsig_plan_create_capped: k_capped_tiles; k_capped_scan and k_capped_cover for the
coverage form), the two file-level calls and the keyword of bamCount / bamProfile / bamCoverage -- against the definition
(tests/capped_expected.py: the C oracle's per-base stranded cells, np.minimum, reduceat, window sums).  All exact."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN

import capped_expected as ce
from test_depthhist_gpu import REF_LEN, _cat, _params, _pile, _ranges, _upload, decode_mode, fixture, synth  # noqa: F401

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
HUGE = 2 ** 31 - 1
PILE_STEP = 4999            # a pile of 8 reads every so many bases, on alternating strands: 8 = 5 + 3 is above every k of the grid


def _mode(binsize):
    from bamsignals_amd import _lib
    return _lib.MODE_COUNT if binsize <= 0 else _lib.MODE_PROFILE


def _capped(ctx, reads, rg, k, binsize=1, ss=False, runs=2, frag_len=0, **kw):
    """a capped plan's first run and its later ones, which must agree; (flat int32 result, offsets, stats, runs)"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import CappedPlan, make_params
    if frag_len:
        p = make_params(_lib.MODE_COVERAGE_EX, binsize=binsize, ss=ss, **kw)
    else:
        p = make_params(_mode(binsize), binsize=binsize, ss=ss, **kw)
    plan = CappedPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], p, k, frag_len)
    try:
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int32 and got[0].shape == (plan.cells,) and plan.cells == plan.offsets[-1]
        return got[0], plan.offsets, plan.stats(), plan.runs
    finally:
        plan.close()


def _same(got, goff, want, woff, what):
    assert np.array_equal(goff, woff), what
    bad = np.flatnonzero(got != want)[:6]
    assert bad.size == 0, (what, bad.tolist(), got[bad].tolist(), want[bad].tolist())


@pytest.fixture(scope="module")
def piled(synth):
    """the synthetic reads with a pile of 8 reads every PILE_STEP bases of both references, resident on GPU 0"""
    ctx, bg, _, _ = synth
    ref_off = np.asarray(bg["ref_off"])
    parts = [dict(rid=np.repeat(np.arange(2), np.diff(ref_off)), pos=bg["pos"], end=bg["end"], flag=bg["flag"], mapq=bg["mapq"],
                  tlen=bg["tlen"])]
    for rid, n in enumerate(REF_LEN):
        for j, at in enumerate(range(PILE_STEP, n - 100, PILE_STEP)):
            parts.append(ce.planted(8, 0, at, rid=rid, reverse=bool(j % 2)))
    cols = ce.merge_sorted(parts, 2)
    cols["ref_len"] = np.asarray(REF_LEN, np.int64)
    reads = _upload(ctx, cols)
    yield ctx, cols, reads, ce.oracle_reads(cols)
    reads.close()


def _on_piles(w, n=6):
    """ranges of width w that hold a pile each, on the three strands"""
    at = PILE_STEP * (3 + np.arange(n))
    return dict(rid=np.zeros(n, np.int32), loc=(at - np.minimum(w - 1, 3)).astype(np.int32), len=np.full(n, w, np.int32),
                strand=np.asarray([1, -1, 0] * n, np.int32)[:n])


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [None, "64"])
@pytest.mark.parametrize("w", [1, 100, 2048, 2049, 10_000])
def test_grid(piled, w, heavy, monkeypatch):
    ctx, cols, reads, orc = piled
    if heavy:
        monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", heavy)
    rg = _cat(_ranges(60 if w < 10_000 else 12, w, seed=w), _on_piles(w))
    assert len(set(rg["strand"].tolist())) == 3
    cells = ce.stranded_cells(orc, rg)
    flat = np.concatenate([c.reshape(-1) for c in cells])
    heavy_seen = 0
    for k in (1, 2, 5):
        # (not vacuous, on the expected side first)
        assert (flat > k).any() and ((flat > 0) & (flat <= k)).any()
        for binsize in (1, 7, 200, w + 10, -1):
            for ss in (False, True):
                want, woff = ce.ends_from_cells(cells, k, binsize, ss)
                got, goff, st, n_runs = _capped(ctx, reads, rg, k, binsize, ss)
                _same(got, goff, want, woff, (w, k, binsize, ss, heavy))
                assert st["cells"] == got.size and n_runs >= st["heavy_tiles"]
                heavy_seen += st["heavy_tiles"]
    # (which image ran: none is wide without the lowered ceiling; with it every tile of 2,048 bases is)
    assert heavy_seen == 0 if heavy is None else (w < 2048 or heavy_seen > 0)


def test_the_largest_cap_is_the_plain_plan(piled):
    from bamsignals_amd.device import Plan, make_params
    ctx, cols, reads, orc = piled
    rg = _cat(_ranges(40, 3000, seed=5, jitter=2900), _on_piles(700), dict(rid=[1], loc=[30], len=[0], strand=[-1]))
    for binsize, ss, shift in ((1, True, 0), (1, False, 0), (7, True, 33), (200, False, -70), (5000, True, 0), (-1, True, 5), (-1, False, 0)):
        plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_mode(binsize), binsize=binsize, ss=ss, shift=shift))
        want = plan.run_host()
        woff = plan.offsets
        plan.close()
        got, goff, _, _ = _capped(ctx, reads, rg, HUGE, binsize, ss, shift=shift)
        _same(got, goff, want, woff, (binsize, ss, shift))
        assert want.max() >= 8


# ---- seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_tiles", [None, "1"])
def test_seams(synth, run_tiles, monkeypatch):
    """tiles of 64 cells: bins of 50 straddle tiles, bins of 1000 hold several; piles of k + 3 on the last base of a tile and
    the first of the next, on both strands, in '+' and '-' ranges; every tile its own run"""
    ctx = synth[0]
    if run_tiles:
        monkeypatch.setenv("BAMSIGNALS_CAPPED_RUN_TILES", run_tiles)
    loc, w, k = 40_000, 64 * 40 + 17, 2
    parts = []
    for strand in (1, -1):
        for x in (0, 63, 64, 127, 128, 999, 1000, 64 * 39 + 63, 64 * 40, w - 1):
            g = loc + x if strand > 0 else loc + w - 1 - x
            parts += [ce.planted(k + 3, 0, g, read_len=1), ce.planted(k + 3, 0, g, reverse=True, read_len=1)]
    for x in (7, 73, 1500, w - 30):
        parts += [ce.planted(1, 0, loc + x, read_len=1), ce.planted(2, 0, loc + x, reverse=True, read_len=1)]
    cols = ce.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=[0, 0, 0], loc=[loc, loc, loc + 5], len=[w, w, 300], strand=[1, -1, -1])
        cells = ce.stranded_cells(cols, rg)
        assert max(int(c.max()) for c in cells) >= k + 3
        for binsize in (1, 50, 1000, -1):
            for ss in (False, True):
                for threads in (64, 256):
                    want, woff = ce.ends_from_cells(cells, k, binsize, ss)
                    got, goff, st, n_runs = _capped(ctx, reads, rg, k, binsize, ss, tile_cells=64, threads=threads)
                    _same(got, goff, want, woff, (binsize, ss, threads, run_tiles))
                    assert st["n_items"] == 2 * 41 + 5
                    if run_tiles:
                        assert n_runs == st["n_items"]
    finally:
        reads.close()


# ---- the 16-bit cell -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65_535, 65_536])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("beside", [False, True])
def test_piles_around_the_16_bit_cell(synth, n, reverse, beside):
    ctx = synth[0]
    cols, reads, rg = _pile(ctx, n, beside, reverse=reverse)
    try:
        cells = ce.stranded_cells(cols, rg)
        top = max(int(c.max()) for c in cells)
        assert top == n if not beside else n <= top <= n + 20       # (a neighbour may share the pile's base)
        for k in (1, 70_000):
            for binsize, ss in ((1, True), (1, False), (100, True), (-1, False)):
                want, woff = ce.ends_from_cells(cells, k, binsize, ss)
                got, goff, st, _ = _capped(ctx, reads, rg, k, binsize, ss)
                _same(got, goff, want, woff, (n, reverse, beside, k, binsize, ss))
                assert st["heavy_tiles"] >= 1           # more reads than a 16-bit image may see: the 32-bit image ran
        assert int(ce.ends_from_cells(cells, 70_000, -1, False)[0][0]) >= n
    finally:
        reads.close()


# ---- packed forms, shift -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"BAMSIGNALS_PACKED_HALF": "0"}, {"BAMSIGNALS_PACK": "0"}], ids=["half", "words", "unpacked"])
def test_packed_forms(piled, env, monkeypatch):
    ctx, cols, _, orc = piled
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    reads = _upload(ctx, cols)
    try:
        rg = _cat(_ranges(30, 3000, seed=11, jitter=1000), _on_piles(900))
        for shift in (0, 25):
            cells = ce.stranded_cells(orc, rg, shift=shift)
            for binsize, ss in ((1, True), (7, False), (-1, True)):
                want, woff = ce.ends_from_cells(cells, 2, binsize, ss)
                got, goff, st, _ = _capped(ctx, reads, rg, 2, binsize, ss, shift=shift)
                _same(got, goff, want, woff, (env, shift, binsize, ss))
                assert st["bytes_per_visit_packed"] == (2 if not env else 4)
    finally:
        reads.close()


@pytest.mark.parametrize("shift", [-70, -1, 1, 70])
def test_shift(piled, shift, monkeypatch):
    ctx, cols, reads, orc = piled
    rg = _cat(_ranges(30, 2500, seed=shift + 100), _on_piles(300))
    rg["strand"][::2] = -1
    cells = ce.stranded_cells(orc, rg, shift=shift)
    unshifted = ce.stranded_cells(orc, rg)
    assert any(not np.array_equal(a, b) for a, b in zip(cells, unshifted))
    for binsize, ss in ((1, True), (1, False), (50, True), (-1, True)):
        want, woff = ce.ends_from_cells(cells, 2, binsize, ss)
        got, goff, st, _ = _capped(ctx, reads, rg, 2, binsize, ss, shift=shift)
        _same(got, goff, want, woff, (shift, binsize, ss))
        assert st["heavy_tiles"] == 0
    # once on wide tiles: the read-by-read body honours the shift too
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    want, woff = ce.ends_from_cells(cells, 2, 1, True)
    got, goff, st, _ = _capped(ctx, reads, rg, 2, 1, True, shift=shift)
    _same(got, goff, want, woff, (shift, "wide"))
    assert st["heavy_tiles"] > 0


# ---- edges and order ---------------------------------------------------------------------------------------------------
def test_edges(piled):
    ctx, cols, reads, orc = piled
    for binsize, ss in ((1, True), (10, False), (-1, True)):
        got, off, st, n_runs = _capped(ctx, reads, dict(rid=[], loc=[], len=[], strand=[]), 1, binsize, ss)
        assert got.size == 0 and off.tolist() == [0] and st["n_items"] == 0 and n_runs == 0
        rg = dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1])
        got, off, _, n_runs = _capped(ctx, reads, rg, 1, binsize, ss)
        assert not got.any() and n_runs == 0 and got.size == (0 if binsize > 0 else (4 if ss else 2))
        # wholly outside the reference, and over both of its ends
        rg = dict(rid=[0, 1, 1], loc=[-500, 705_017, -300], len=[400, 100, REF_LEN[1] + 900], strand=[1, -1, -1])
        want, woff = ce.ends(orc, rg, 2, binsize, ss)
        got, goff, _, _ = _capped(ctx, reads, rg, 2, binsize, ss)
        _same(got, goff, want, woff, (binsize, ss))
        assert got[goff[2]:].sum() > 0 and not got[:goff[2]].any()


def test_a_shuffled_deck_gives_the_shuffled_rows(piled):
    ctx, cols, reads, orc = piled
    rg = _cat(_ranges(50, 3000, seed=3, jitter=2900), dict(rid=[0, 1], loc=[70, 80], len=[0, 5000], strand=[1, -1]))
    perm = np.random.default_rng(8).permutation(len(rg["len"]))
    shuffled = {k: v[perm] for k, v in rg.items()}
    for binsize, ss, L in ((1, True, 0), (30, False, 0), (-1, True, 0), (1, False, 150), (30, True, 150)):
        a, aoff, _, _ = _capped(ctx, reads, rg, 2, binsize, ss, frag_len=L)
        b, boff, _, _ = _capped(ctx, reads, shuffled, 2, binsize, ss, runs=1, frag_len=L)
        for j, i in enumerate(perm):
            assert np.array_equal(b[boff[j]:boff[j + 1]], a[aoff[i]:aoff[i + 1]])
        assert a.sum() > 1000


# ---- the coverage form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 40, 200, 5000])
def test_coverage_form(piled, L):
    """L above a tile (2,048) and above the ranges' width; ranges that start on base 0 and overhang the reference's end"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, cols, reads, orc = piled
    rg = _cat(_ranges(14, 1500, seed=L, jitter=1400), _on_piles(500),
              dict(rid=[0, 1, 1, 0, 0], loc=[0, 0, REF_LEN[1] - 300, 17, 9000], len=[700, 3000, 900, 2500, 0], strand=[1, -1, -1, -1, 1]))
    rg["strand"][1:14:2] = -1
    for binsize in (1, 50):
        for ss in (False, True):
            for k in (1, 2):
                want, woff = ce.coverage(orc, rg, k, L, binsize, ss)
                got, goff, st, _ = _capped(ctx, reads, rg, k, binsize, ss, frag_len=L)
                _same(got, goff, want, woff, (L, binsize, ss, k))
                assert st["cells"] == got.size and got.sum() > 0
            # the largest cap: the existing resized coverage plan
            plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"],
                        make_params(_lib.MODE_COVERAGE_EX, binsize=binsize, ss=ss), frag_len=L)
            want, woff = plan.run_host(), plan.offsets
            plan.close()
            got, goff, _, _ = _capped(ctx, reads, rg, HUGE, binsize, ss, frag_len=L)
            _same(got, goff, want, woff, (L, binsize, ss, "resized"))
    # on wide tiles and tiles of 64 cells
    want, woff = ce.coverage(orc, rg, 2, L, 1, True)
    got, goff, _, _ = _capped(ctx, reads, rg, 2, 1, True, frag_len=L, tile_cells=64)
    _same(got, goff, want, woff, (L, "tile 64"))


def test_coverage_form_on_wide_tiles(piled, monkeypatch):
    ctx, cols, reads, orc = piled
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    rg = _cat(_ranges(10, 4000, seed=77), _on_piles(3000))
    want, woff = ce.coverage(orc, rg, 2, 180, 1, True)
    got, goff, st, _ = _capped(ctx, reads, rg, 2, 1, True, frag_len=180)
    _same(got, goff, want, woff, "wide")
    assert st["heavy_tiles"] > 0


# ---- another kind agrees ---------------------------------------------------------------------------------------------
def test_the_depth_histogram_gives_the_same_total(piled):
    from bamsignals_amd.device import HistPlan
    ctx, cols, reads, orc = piled
    rg = _cat(_ranges(40, 3000, seed=9, jitter=2000), _on_piles(1000))
    hp = HistPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params("ends", True), 100)
    hist = hp.run_host()[:101]
    hp.close()
    assert hist[100] == 0 and hist[8:].sum() > 0
    v = np.arange(101)
    for k in (1, 2, 5, 50):
        got, _, _, _ = _capped(ctx, reads, rg, k, 1, True, runs=1)
        assert int(got.astype(np.int64).sum()) == int((np.minimum(v, k) * hist).sum())


# ---- errors and plan kinds ---------------------------------------------------------------------------------------------
def test_errors(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import CappedPlan, make_params
    ctx, cols, reads, _ = synth
    a = ([0], [10], [100], [1])
    paired = "a paired-end duplicate is a fragment with both ends equal, which a 5' end and a strand do not identify: %s must be 0 with keep_dup"
    P, CNT, COV, EX = _lib.MODE_PROFILE, _lib.MODE_COUNT, _lib.MODE_COVERAGE, _lib.MODE_COVERAGE_EX
    for p, k, L, message in (
            (make_params(P), 0, 0, "keep_dup must be at least 1 (0 given)"),
            (make_params(CNT, binsize=-1), -5, 0, "keep_dup must be at least 1 (-5 given)"),
            (make_params(P, pe_mid=True, tlen_filter=(0, 500)), 1, 0, paired % "pe_mid"),
            (make_params(EX, tspan=True, tlen_filter=(0, 500)), 1, 100, paired % "tspan"),
            (make_params(P, tlen_filter=(0, 500)), 1, 0, "keep_dup caps single-end reads: it takes no template-length rule (n_tlen_filter must be 0)"),
            (make_params(COV), 1, 0, "duplicates of different lengths have no defined survivor: bamCoverage takes keep_dup with a fragment length only"),
            (make_params(P), 1, 100, "reads are resized to the fragment for bamCoverage only (mode 0 given): frag_len must be 0"),
            (make_params(EX), 1, -1, "the fragment length must be between 1 and 16777216 (-1 given)"),
            (make_params(EX), 1, (1 << 24) + 1, "the fragment length must be between 1 and 16777216 (16777217 given)"),
            (make_params(EX, binsize=65537), 1, 10, "coverage bins are at most 65536 bases wide (bamProfile / bamCount count at that scale)"),
            (make_params(P, binsize=0), 1, 0, "provide a binsize greater or equal to 1"),
            (make_params(_lib.MODE_OVERLAP_ANY), 1, 0, "keep_dup is defined on bamProfile, bamCount and bamCoverage (mode 4 given)"),
            (make_params(P, threads=96), 1, 0, "threads must be 64, 128 or 256"),
            (make_params(P, tile_cells=2049), 1, 0, "tile_cells must be between 16 and 2048")):
        with pytest.raises(_lib.BsigError) as e:
            CappedPlan(ctx, reads, *a, p, k, L)
        assert (e.value.code_name, str(e.value)) == ("BSIG_ERR_ARG", message)
    with pytest.raises(_lib.BsigError) as e:
        CappedPlan(ctx, reads, [5], [10], [100], [1], make_params(P), 1)
    assert e.value.code_name == "BSIG_ERR_CHROM"
    with pytest.raises(_lib.BsigError, match="negative width"):
        CappedPlan(ctx, reads, [0], [10], [-1], [1], make_params(EX), 1, 50)
    with pytest.raises(_lib.BsigError, match="ends beyond 2\\^31 - 1"):
        CappedPlan(ctx, reads, [0], [HUGE - 600], [502], [1], make_params(EX), 1, 100)
    for tile, k in ((16, 1), (2048, HUGE)):
        CappedPlan(ctx, reads, *a, make_params(P, tile_cells=tile), k).close()


def test_stale_plan_and_wrong_run_calls(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import CappedPlan, HistPlan, Plan, ScaledPlan, SumPlan, make_params
    ctx, cols, _, _ = synth
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        a = ([0], [10], [100], [1])
        prof = make_params(_lib.MODE_PROFILE)
        cp = CappedPlan(ctx, reads, *a, prof, 1)
        cc = CappedPlan(ctx, reads, *a, make_params(_lib.MODE_COVERAGE_EX, ss=True), 1, 60)
        pp, sp = Plan(ctx, reads, *a, prof), SumPlan(ctx, reads, *a, prof)
        hp = HistPlan(ctx, reads, *a, _params("coverage", False), 24)
        mp = ScaledPlan(ctx, reads, *a, _params("coverage", False), 5)
        b32, b64 = np.zeros(400, np.int32), np.zeros(400, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        host, dev = "a capped plan runs with bsig_plan_run_capped_host", "a capped plan runs with bsig_plan_run_capped"
        for fn, plan, buf, says in (
                (lib.bsig_plan_run_host, cp, p32, host),
                (lib.bsig_plan_run, cp, p32, dev),
                (lib.bsig_plan_run_host_async, cc, p32, dev),
                (lib.bsig_plan_run_sum_host, cp, p64, host),
                (lib.bsig_plan_run_sum, cc, p64, dev),
                (lib.bsig_plan_run_xcorr_host, cp, p64, host),
                (lib.bsig_plan_run_frag, cp, p64, dev),
                (lib.bsig_plan_run_hist_host, cc, p64, host),
                (lib.bsig_plan_run_summary, cp, p64, dev),
                (lib.bsig_plan_run_scaled_host, cp, p64, host),
                (lib.bsig_plan_run_vplot, cc, p64, dev),
                (lib.bsig_plan_run_capped_host, pp, p32, "not a capped plan: bsig_plan_run_host runs it"),
                (lib.bsig_plan_run_capped, pp, p32, "not a capped plan: bsig_plan_run runs it"),
                (lib.bsig_plan_run_capped_host, sp, p32, "not a capped plan: bsig_plan_run_sum_host runs it"),
                (lib.bsig_plan_run_capped, hp, p32, "not a capped plan: bsig_plan_run_hist runs it"),
                (lib.bsig_plan_run_capped_host, mp, p32, "not a capped plan: bsig_plan_run_scaled_host runs it")):
            assert fn(plan._h, buf) == -1
            assert lib.bsig_last_error().decode() == says
        assert not b32.any() and not b64.any()
        h = C.c_void_p()
        assert lib.bsig_plan_runs_create(cp._h, C.byref(h)) == -1
        assert lib.bsig_last_error().decode() == "a capped plan has no per-range result to encode"
        for other in (pp, sp, hp, mp):
            assert lib.bsig_plan_capped_cells(other._h) == 0 and lib.bsig_plan_capped_runs(other._h) == 0
        assert lib.bsig_plan_capped_cells(cp._h) == 100 and lib.bsig_plan_capped_cells(cc._h) == 200
        assert lib.bsig_plan_cells(cc._h) == 200 and lib.bsig_plan_scaled_cells(cp._h) == 0 and lib.bsig_plan_sum_cells(cc._h) == 0
        first, cov = cp.run_host(), cc.run_host()
        assert first.max() == 1 and cov.sum() > 0
        assert np.array_equal(cp.run_host(), first) and np.array_equal(cc.run_host(), cov)
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        for plan in (cp, cc):
            with pytest.raises(_lib.BsigError, match="make a new plan"):
                plan.run_host()
        cp2 = CappedPlan(ctx, reads, *a, prof, 1)
        assert np.array_equal(cp2.run_host(), first)
        for p in (cp, cc, cp2, pp, sp, hp, mp):
            p.close()
    finally:
        reads.close()


# ---- file level ------------------------------------------------------------------------------------------------------
def test_file_level(fixture, decode_mode):
    from bamsignals_amd import bamCount, bamCoverage, bamProfile
    gr, rg, cols, whole, whole_rg = fixture
    orc = ce.oracle_reads(cols)
    n = len(rg["len"])
    for k in (1, 3):
        for ss in (False, True):
            for binsize, shift in ((1, 0), (25, 40)):
                want, woff = ce.ends(orc, rg, k, binsize, ss, shift=shift)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")         # (widths that are no multiple of the binsize)
                    sig = bamProfile(BAM, gr, binsize=binsize, shift=shift, ss=ss, keepDup=k, verbose=False)
                for i in range(n):
                    w = want[woff[i]:woff[i + 1]]
                    assert np.array_equal(np.asarray(sig[i]), w.reshape(-1, 2).T if ss else w), (k, ss, binsize, i)
            want, _ = ce.ends(orc, rg, k, -1, ss)
            cnt = bamCount(BAM, gr, ss=ss, keepDup=k, verbose=False)
            assert np.array_equal(cnt, want.reshape(-1, 2).T if ss else want) and cnt.dtype == np.int32
            for L, binsize in ((150, 1), (37, 10)):
                want, woff = ce.coverage(orc, rg, k, L, binsize, ss)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sig = bamCoverage(BAM, gr, fragLength=L, keepDup=k, binsize=binsize, ss=ss, verbose=False)
                for i in range(n):
                    w = want[woff[i]:woff[i + 1]]
                    assert np.array_equal(np.asarray(sig[i]), w.reshape(-1, 2).T if ss else w), (k, ss, L, binsize, i)
    # whole chromosomes; the cap bites (the fixture's largest stranded cell is 11, 9 and 10)
    a = bamProfile(BAM, whole, ss=True, keepDup=2, verbose=False)
    b = bamProfile(BAM, whole, ss=True, verbose=False)
    for i in range(3):
        assert np.array_equal(np.asarray(a[i]), np.minimum(np.asarray(b[i]), 2)) and np.asarray(b[i]).max() > 2
    # keepDup=None is the call of always
    assert np.array_equal(np.asarray(bamProfile(BAM, whole, ss=True, keepDup=None, verbose=False)[0]), np.asarray(b[0]))


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import _lib, bamCount, bamCoverage, bamProfile
    from bamsignals_amd.wrappers import last_call_route
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    calls = (lambda: bamProfile(BAM, gr, ss=True, keepDup=1, verbose=False),
             lambda: bamCount(BAM, gr, keepDup=2, shift=10, verbose=False),
             lambda: bamCoverage(BAM, gr, fragLength=120, keepDup=1, ss=True, verbose=False))
    try:
        for call in calls:
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
            one = call()
            assert "1 GPU slot(s)" in last_call_route() and "capped" in last_call_route()
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
            four = call()
            assert "capped of 4 blocks of ranges, rows placed on the host" in last_call_route()
            if isinstance(one, np.ndarray):
                assert np.array_equal(one, four) and one.any()
            else:
                assert all(np.array_equal(np.asarray(one[i]), np.asarray(four[i])) for i in range(len(gr)))
                assert sum(int(np.asarray(s).sum()) for s in one) > 0
    finally:
        _lib.load().bsig_cache_clear()


# ---- the use ---------------------------------------------------------------------------------------------------------
def test_user_level_on_a_written_bam(piled, tmp_path):
    """MACS's pileup: --keep-dup 1 and --extsize from the data's own cross-correlation"""
    from bamsignals_amd import GRanges, _lib, bamCount, bamCoverage, bamCrossCorr, bamProfile, write_columns_as_bam
    ctx, cols, _, orc = piled
    bam = str(tmp_path / "piled.bam")
    cig = dict(cigar_off=np.arange(len(cols["pos"]) + 1, dtype=np.int64),
               cigar=((cols["end"].astype(np.int64) - cols["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(bam, ["chrA", "chrB"], dict(cols, **cig))
    try:
        rg = _cat(_ranges(30, 2000, seed=4), _on_piles(800))
        gr = GRanges([("chrA", "chrB")[r] for r in rg["rid"]], rg["loc"] + 1, width=rg["len"],
                     strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in rg["strand"]])
        n = len(rg["len"])
        want, off = ce.ends(orc, rg, 1, 1, True)
        sig = bamProfile(bam, gr, keepDup=1, ss=True, verbose=False)
        assert all(np.array_equal(np.asarray(sig[i]), want[off[i]:off[i + 1]].reshape(-1, 2).T) for i in range(n))
        assert max(int(np.asarray(s).max()) for s in sig) == 1
        want, _ = ce.ends(orc, rg, 2, -1, False)
        assert np.array_equal(bamCount(bam, gr, keepDup=2, verbose=False), want)
        L = bamCrossCorr(bam, gr, verbose=False).fragment_length()
        assert 1 <= L <= 1 << 24
        want, off = ce.coverage(orc, rg, 1, L)
        cov = bamCoverage(bam, gr, fragLength=L, keepDup=1, verbose=False)
        assert all(np.array_equal(np.asarray(cov[i]), want[off[i]:off[i + 1]]) for i in range(n))
        plain = bamCoverage(bam, gr, fragLength=L, verbose=False)
        assert sum(int(np.asarray(s).sum()) for s in cov) < sum(int(np.asarray(s).sum()) for s in plain)
    finally:
        _lib.load().bsig_cache_clear()
