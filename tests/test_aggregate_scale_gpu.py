"""GPU: sums over ranges (bsig_plan_create_sum: k_sum_tiles, k_sum_reduce, k_sum_scan, k_sum_bins) where a wave takes
many DIFFERENT tiles, where a run is as long as it may get, and on the reads and ranges of the parameter extremes.

Expected values: the C oracle per range, summed over the ranges in int64 (in blocks of ranges), coverage binned and
split by strand as test_aggregate_gpu.want_coverage does.  Never the per-range plan of the library.

1. test_forced_runs / test_tile_cells_of_the_caller: the run length of a sum plan forced (BAMSIGNALS_SUM_RUN_TILES) to
   1, 2, 3, 5, 64 and 1,000 tiles on 600 distinct ranges, so that the waves of a workgroup fold, clear and go on to
   other items, other kept windows and other strands; every read form, three runs and one without kept windows, with
   and without heavy slices; tile sizes of the caller's.
2. test_default_cut_at_scale: the occupancy-derived cut at 30,000 to 300,000 ranges on 4,100,000 reads: at least 8
   tiles per wave and more than 32 runs (several k_sum_reduce chunks) per tile position, both proven from the device.
3. test_slab_*: runs of 65,536 tiles over piles of 32,768 (32,767) reads: slab cells of 2^31 (+-(2^31 - 65,536)), and
   the clamp of the run length.
4. test_extremes_*: one sum plan per width of extremes_inputs.place_ranges at megabase shifts, midpoints and template
   spans, with the half form on the side the documented bound puts it.

Mismatches are collected and reported together (test_parameter_extremes_gpu._summary).
"""
import time

import numpy as np
import pytest

import aggregate_scale_inputs as S
import extremes_inputs as X
import test_aggregate_gpu as A
from test_parameter_extremes_gpu import FAR_H, _hs, _summary

pytestmark = pytest.mark.gpu

RUN_ENV = "BAMSIGNALS_SUM_RUN_TILES"
MAX_RUN = 65_536


# ---------------------------------------------------------------------------------------------------------------
# expected values and runs
# ---------------------------------------------------------------------------------------------------------------
def want_sum(cols, rg, kind, b, ss, kw, cells=20_000_000):
    """the oracle per range, summed in int64 over blocks of ranges of at most `cells` per-base cells"""
    n, w = len(rg["len"]), int(rg["len"][0])
    step = max(1, cells // max(w, 1))
    tot = None
    for a in range(0, n, step):
        part = S.take(rg, slice(a, a + step))
        v = A.want_profile(cols, part, b, ss, **kw) if kind == "profile" else A.want_coverage(cols, part, b, ss, **kw)
        tot = v if tot is None else tot + v
    return tot


def _params(kind, b, ss, kw, threads=0, tile_cells=0):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    mode = {"profile": _lib.MODE_PROFILE, "cov2": _lib.MODE_COVERAGE, "covex": _lib.MODE_COVERAGE_EX}[kind]
    return make_params(mode, binsize=b, ss=ss, threads=threads, tile_cells=tile_cells, **kw)


def _sum_runs(ctx, reads, rg, prm, runs=3, uncached=False, env=None):
    """A sum plan made under `env` (the knobs read when a plan is made) and run `runs` times -- first run fused or with
    the lookup launch, later runs on kept windows -- and, with `uncached`, once more looking its windows up again.
    Returns (results, stats)."""
    from bamsignals_amd.device import SumPlan
    mp = pytest.MonkeyPatch()
    try:
        for k, v in (env or {}).items():
            mp.setenv(k, str(v))
        plan = SumPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], prm)
    finally:
        mp.undo()
    try:
        got = [plan.run_host() for _ in range(runs)]
        if uncached:
            mp.setenv("BAMSIGNALS_CACHE_WINDOWS", "0")
            try:
                got.append(plan.run_host())
            finally:
                mp.undo()
        return got, plan.stats()
    finally:
        plan.close()


def _compare(bad, desc, form, got, want, ss):
    for k, g in enumerate(got):
        g = A._shape(g, ss)
        if g.shape != want.shape or not np.array_equal(g, want):
            bad.append((desc, "%s run=%d" % (form, k + 1), int(np.sum(g != want)) if g.shape == want.shape else -1))


def _desc(kind, b, ss, kw, **more):
    return dict(kind=kind, binsize=b, ss=ss, **kw, **more)


# ---------------------------------------------------------------------------------------------------------------
# 1. runs of many distinct tiles, forced
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    """the reads of test_aggregate_gpu.py resident in every form: {(paired, form): reads}, {paired: columns}"""
    from bamsignals_amd.device import Context
    ctx = Context(0)
    cols = {p: S.grid_reads(p) for p in (False, True)}
    reads = {}
    mp = pytest.MonkeyPatch()
    try:
        reads[False, "half"] = A._reads(ctx, cols[False])
        reads[True, "half"] = A._reads(ctx, cols[True])
        mp.setenv("BAMSIGNALS_PACKED_HALF", "0")
        reads[False, "PACKED_HALF=0"] = A._reads(ctx, cols[False])
        mp.undo()
        mp.setenv("BAMSIGNALS_PACK", "0")
        reads[False, "PACK=0"] = A._reads(ctx, cols[False])
    finally:
        mp.undo()
    assert reads[False, "half"].info()["class_n"][4] > 0 and reads[False, "PACK=0"].info()["class_n"][4] == 0
    yield ctx, cols, reads
    for r in reads.values():
        r.close()
    ctx.close()


def _grid_forms(paired, kind):
    # profiles on every form of the single-end reads; coverage never reads the 16-bit column
    if paired:
        return ("half",)
    return ("half", "PACKED_HALF=0", "PACK=0") if kind == "profile" else ("half", "PACK=0")


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("heavy", [False, True], ids=["", "heavy=64"])
@pytest.mark.parametrize("w", S.GRID_WIDTHS)
def test_forced_runs(grid, w, heavy):
    """Run lengths 1, 2, 3, 5, 64 and 1,000 x threads 64, 128, 256 on 600 distinct ranges of one width: every wave of
    a run takes several tiles of different ranges and strands.  Each plan runs three times and once more without its
    kept windows; with BAMSIGNALS_HEAVY_READS=64 the runs of heavy slices hold many slices per wave as well."""
    ctx, cols, reads = grid
    rg = S.grid_ranges(w)
    env = {"BAMSIGNALS_HEAVY_READS": 64} if heavy else {}
    bad, n_plans = [], 0
    for paired in (False, True):
        for kind, b, ss, kw in S.grid_cases(paired):
            want = want_sum(cols[paired], rg, kind, b, ss, kw)
            assert want.sum() > 0
            for form in _grid_forms(paired, kind):
                for run in S.RUN_TILES:
                    for th in S.THREADS:
                        got, st = _sum_runs(ctx, reads[paired, form], rg, _params(kind, b, ss, kw, threads=th), runs=3,
                                            uncached=True, env=dict(env, **{RUN_ENV: run}))
                        n_plans += 1
                        assert st["n_ranges"] == S.GRID_RANGES and st["n_items"] >= S.GRID_RANGES
                        assert (st["heavy_tiles"] > 0) == heavy, (kind, b, ss, form, st["heavy_tiles"])
                        if kind == "profile":
                            # the 16-bit column: per-base tiles, no template-length rule, the column laid out
                            assert (st["bytes_per_visit_packed"] == 2) == (form == "half" and not paired), (form, paired, st)
                        _compare(bad, _desc(kind, b, ss, kw, w=w, paired=paired), "%s run_tiles=%d threads=%d" % (form, run, th),
                                 got, want, ss)
    assert n_plans == (4 * 3 + 3 * 2 + 7) * len(S.RUN_TILES) * len(S.THREADS)
    assert not bad, _summary(bad)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("w", [2_049, 10_000])
def test_tile_cells_of_the_caller(grid, w):
    """Tile sizes given by the caller (64, 68, 1,000, 4,096: each a multiple of 4 and at least 64, which
    plan_create_impl takes as they are) at run length 5.  A size whose accumulator and images do not fit a workgroup's
    LDS (strand-split coverage at 4,096 cells with four waves asks for 164,352 bytes of 163,840) must make the plan
    take fewer waves or be refused with BSIG_ERR_ARG when the plan is made: every plan that is made gives the oracle's
    sum, and only the largest size may be refused."""
    from bamsignals_amd import _lib
    ctx, cols, reads = grid
    rg = S.grid_ranges(w)
    bad, refused, made = [], [], 0
    for paired in (False, True):
        for kind, b, ss, kw in S.grid_cases(paired):
            want = want_sum(cols[paired], rg, kind, b, ss, kw)
            for tc in S.TILE_CELLS:
                for th in (64, 256):
                    try:
                        got, st = _sum_runs(ctx, reads[paired, "half"], rg, _params(kind, b, ss, kw, threads=th, tile_cells=tc),
                                            runs=3, uncached=True, env={RUN_ENV: 5})
                    except _lib.BsigError as e:
                        # only when the plan is made (a failing run is not caught: _sum_runs made the plan by then)
                        assert e.code_name == "BSIG_ERR_ARG" and "LDS" in str(e), str(e)
                        refused.append((kind, ss, tc, th))
                        continue
                    made += 1
                    assert st["n_items"] == S.GRID_RANGES * -(-w // tc)
                    _compare(bad, _desc(kind, b, ss, kw, w=w, paired=paired), "tile_cells=%d threads=%d" % (tc, th), got, want, ss)
    assert all(tc == max(S.TILE_CELLS) for _, _, tc, _ in refused), refused
    assert made >= 14 * 2 * (len(S.TILE_CELLS) - 1)
    assert not bad, _summary(bad)


# ---------------------------------------------------------------------------------------------------------------
# 2. the default cut at the sizes sum plans were built for
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scale():
    from bamsignals_amd.device import Context, Reads
    ctx = Context(0)
    cols = S.scale_reads()
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    yield ctx, cols, reads
    reads.close()
    ctx.close()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("n,w", S.SCALE_SHAPES, ids=lambda v: str(v))
def test_default_cut_at_scale(scale, n, w):
    """The library's own cut (run-length knob unset) at 300,000 x 200, 60,000 x 2,049 (with strands: tiles of 1,024,
    1,024 and 1 cells) and 30,000 x 10,000 on 4,000,000 paired reads and a pile of 100,000: threads 64 and 256, two
    runs.  The guards use the device alone.  At most 32 waves are resident per CU, so every full run holds at least
    n_items * nw / (32 CUs') tiles: at least 8 per wave for the 300,000-range shape.  At least one workgroup is
    resident per CU, so a run holds at most ceil(n_items / CUs) tiles and a tile position of n tiles has at least
    n / ceil(n_items / CUs) runs: more than 32 (one k_sum_reduce chunk) for every shape on its 2,048-cell tiles.  The
    strand-split plans cut tiles of 1,024 cells, twice as many, which halves that figure (25.6 for 30,000 x 10,000 on
    256 CUs); their workgroups need at most 24.5 KiB of the CU's 160 KiB of LDS and 4 of its 32 waves, so at least two
    are resident per CU and the bound is taken with two."""
    import os

    import torch
    assert not os.environ.get(RUN_ENV)
    ctx, cols, reads = scale
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    rg = S.scale_ranges(n, w)
    assert set(np.unique(rg["strand"])) == {-1, 0, 1}
    bad = []
    for kind, b, ss, kw in S.SCALE_CASES:
        t0 = time.time()
        want = want_sum(cols, rg, kind, b, ss, kw)
        print("oracle %s ss=%d %d x %d: %.1f s, largest sum %d" % (kind, ss, n, w, time.time() - t0, want.max()))
        assert want.max() > 0
        for th in (64, 256):
            got, st = _sum_runs(ctx, reads, rg, _params(kind, b, ss, kw, threads=th), runs=2)
            nw, items = th // 64, st["n_items"]
            assert st["n_ranges"] == n and items >= 32_768 and items % n == 0      # the resolved form from the first run
            assert st["heavy_tiles"] > 0
            if (n, w) == S.SCALE_SHAPES[0]:
                assert items * nw / (cu * 32) >= 8, (items, nw, cu)
            wg_per_cu = 2 if ss else 1
            runs_per_c0 = n / -(-items // (cu * wg_per_cu))
            assert runs_per_c0 > 32, (n, items, cu, runs_per_c0)
            _compare(bad, _desc(kind, b, ss, kw, n=n, w=w), "threads=%d" % th, got, want, ss)
    assert not bad, _summary(bad)


# ---------------------------------------------------------------------------------------------------------------
# 3. the slab bound and the cap
# ---------------------------------------------------------------------------------------------------------------
N_SLAB = 131_077
LOC = 49_990


def _one(loc, strand):
    return dict(rid=np.zeros(1, np.int32), loc=np.asarray([loc], np.int32), len=np.asarray([64], np.int32),
                strand=np.asarray([strand], np.int32))


def _two_variants():
    """131,077 ranges of 64 bases, alternating '+' at LOC and '-' at LOC + 1: the plan orders its tiles by (reference,
    loc), so the 65,539 '+' ranges come first and the first run of 65,536 tiles holds that variant alone"""
    a, b = _one(LOC, 1), _one(LOC + 1, -1)
    even = (np.arange(N_SLAB) % 2 == 0)
    rg = {k: np.where(even, a[k][0], b[k][0]).astype(np.int32) for k in a}
    return rg, a, b, int(even.sum()), int((~even).sum())


def _slab_case(ctx, n_reads, cases, run_tiles, identical, min_max):
    cols, reads = A._pile(ctx, n_reads, forward=True)
    bad, largest = [], []
    try:
        rg, a, b, n_a, n_b = _two_variants()
        if identical:
            rg, b, n_a, n_b = {k: np.repeat(v, N_SLAB) for k, v in a.items()}, a, N_SLAB, 0
        for kind, ss in cases:
            want = n_a * want_sum(cols, a, kind, 1, ss, {}) + n_b * want_sum(cols, b, kind, 1, ss, {})
            t0 = time.time()
            got, st = _sum_runs(ctx, reads, rg, _params(kind, 1, ss, {}), runs=2, env={RUN_ENV: run_tiles})
            print("%s ss=%d pile=%d run_tiles=%d: plan + 2 runs %.2f s" % (kind, ss, n_reads, run_tiles, time.time() - t0))
            assert st["n_items"] == N_SLAB and st["heavy_tiles"] == 0
            assert want.max() > min_max
            _compare(bad, _desc(kind, 1, ss, {}, pile=n_reads), "run_tiles=%d" % run_tiles, got, want, ss)
            largest.append(int(got[0].max()))
    finally:
        reads.close()
    assert not bad, _summary(bad)
    assert min(largest) > min_max


@pytest.mark.timeout(75)
def test_slab_cell_of_2_to_the_31(grid):
    """Runs of exactly 65,536 tiles over a pile of 32,768 reads (not heavy: the threshold is MORE than 32,768): the
    first run's slab cell is 65,536 x 32,768 = 2^31, negative to anyone who reads it signed.  Profiles with and
    without strands.  Measured on an MI355X: 1.7 s a run (three workgroups, each streaming up to 65,536 x 32,768 reads
    onto one LDS cell), 7.2 s for the test; the time limit is ten times that."""
    assert MAX_RUN * 32_768 == 2**31
    _slab_case(grid[0], 32_768, (("profile", False), ("profile", True)), MAX_RUN, False, 2**31)


@pytest.mark.timeout(220)
def test_slab_cells_of_coverage(grid):
    """The same with 32,767 reads for coverage: slab cells of +-(2^31 - 65,536), the positive one at the pile's first
    base and the negative one after its last.  Per base (mode 2) and split by strand.  Measured: 3.5 s a run per base,
    7 s split by strand, 21.6 s for the test."""
    _slab_case(grid[0], 32_767, (("cov2", False), ("covex", True)), MAX_RUN, False, 2**31)


@pytest.mark.timeout(110)
def test_run_length_is_capped(grid):
    """A run length of 1,000,000 asked for 131,077 identical ranges: held at 65,536 tiles.  One run of all of them
    would give a slab cell of 131,077 x 32,768 = 2^32 + 163,840, which comes back as 163,840 (coverage: past 2^31).
    Measured: 10.8 s for the test."""
    _slab_case(grid[0], 32_768, (("profile", False),), 1_000_000, True, 2**32)
    _slab_case(grid[0], 32_767, (("cov2", False),), 1_000_000, True, 2**31)


# ---------------------------------------------------------------------------------------------------------------
# 4. sum plans on the extremes inputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def extremes(grid):
    """The clustered reads of the parameter extremes, resident with and without the packed class."""
    from bamsignals_amd.device import Reads
    from oracle import oracle_c
    ctx = grid[0]
    cols = X.make_reads()
    mk = lambda: Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])  # noqa: E731
    packed = mk()
    mp = pytest.MonkeyPatch()
    mp.setenv("BAMSIGNALS_PACK", "0")
    try:
        plain = mk()
    finally:
        mp.undo()
    assert packed.info()["class_n"][4] > len(cols["pos"]) // 2 and plain.info()["class_n"][4] == 0
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    yield dict(ctx=ctx, cols=cols, packed=packed, plain=plain, orc=orc)
    packed.close()
    plain.close()


def _extreme_forms(data, rg, kind, b, ss, kw):
    """(form, results of runs 1 and 2, stats, packed?) of every way a sum plan runs this group"""
    for name in ("packed", "plain"):
        for th in (64, 256):
            for run in (0, 3):
                got, st = _sum_runs(data["ctx"], data[name], rg, _params(kind, b, ss, kw, threads=th), runs=2,
                                    env={RUN_ENV: run} if run else None)
                yield "%s threads=%d run_tiles=%s" % (name, th, run or "default"), got, st, name == "packed"


def _half_bound(reads, w, ext):
    """the documented bound of the 16-bit column (plan_create_impl): tile bases + 2 ext + the packed class's longest
    span + two index buckets <= 2^15 - 256; a strand-split sum plan cuts tiles of at most 1,024 cells"""
    inf = reads.info()
    tile = (min(max(w, 64), 1_024) + 3) & ~3
    return tile + 2 * ext + inf["class_maxspan"][4] + 2 * (1 << inf["class_bucket_shift"][4]) <= 2**15 - 256


def _profile_groups(data, rg, rev, a, far_h=None):
    """Every width group of `rg` under bamProfile parameters `a`, per base and in 50-base bins, strands split.
    Returns (mismatches, bytes per packed visit of every plan on the packed reads by width)."""
    from oracle import oracle_c
    bad, sides = [], {}
    groups = S.width_groups(rg)
    for b in (1, 50):
        want, off = oracle_c.pileup_core(data["orc"], rg, binsize=b, ss=True, **a)
        tot, anti, _ = X.rev_hits(want, off, rev, rg["strand"], True)
        assert tot > 0 and anti > 0, ("no reverse-strand read reaches its ranges", a)
        if far_h is not None:
            assert X.rev_hits(want, off, rev, rg["strand"], True, min_h=far_h)[2] > 0
        nonzero = 0
        for w, idx in groups.items():
            w_sum = np.stack([want[off[i]:off[i + 1]] for i in idx]).astype(np.int64).sum(axis=0).reshape(-1, 2).T
            nonzero += bool(w_sum.any())
            for form, got, st, is_packed in _extreme_forms(data, S.take(rg, idx), "profile", b, True, a):
                if is_packed:
                    sides.setdefault(w, set()).add(st["bytes_per_visit_packed"])
                _compare(bad, dict(a, binsize=b, w=w), form, got, w_sum, True)
        assert nonzero >= 4, ("expected sums are zero for most widths", a, b)
    return bad, sides


@pytest.mark.timeout(900)
@pytest.mark.parametrize("shift", S.EXTREME_SHIFTS)
def test_extremes_profile_at_shift(extremes, shift):
    """One sum plan per width (1 to 40,000 bases) of the ranges placed for `shift`.  The 16-bit column is read at
    shift 0 wherever the documented bound allows it and at no megabase shift."""
    rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, shift)
    bad, sides = _profile_groups(extremes, rg, rev, dict(shift=shift))
    if shift == 0:
        for w, s in sides.items():
            assert s == ({2} if _half_bound(extremes["packed"], w, 0) else {4}), (w, s)
        assert any(s == {2} for s in sides.values())
    else:
        assert all(s <= {4, 8} for s in sides.values()) and sides, sides
    assert not bad, _summary(bad)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("shift,tf", S.EXTREME_MIDPOINT, ids=lambda v: str(v))
def test_extremes_midpoint(extremes, shift, tf):
    """paired.end = "midpoint" with template lengths up to 1e9 (ext = 2^30 in the second case): never the 16-bit column"""
    hs = _hs(tf[1])
    rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, shift, hs=hs)
    bad, sides = _profile_groups(extremes, rg, rev, dict(shift=shift, requiredF=66, pe_mid=True, tlen_filter=tf), far_h=FAR_H)
    assert all(s <= {4, 8} for s in sides.values()) and sides, sides
    assert not bad, _summary(bad)


@pytest.mark.timeout(900)
def test_extremes_coverage_with_template_spans(extremes):
    """bamCoverage(paired.end = "extend") with tlen_filter (0, 2e7) summed per width: reads that cover up to 20 Mbp
    start in every tile they cross, which the scan restarted at each tile boundary relies on."""
    from oracle import oracle_c
    data = extremes
    rg, _ = X.place_ranges(X.REFS, X.CLUSTERS, 8_000_000, hs=(0, 4_000_000))
    kw = dict(tspan=True, tlen_filter=X.COVERAGE_TF)
    per, off = oracle_c.coverage_core(data["orc"], rg, **kw)
    starts = np.asarray([c for cl in X.CLUSTERS for c in cl], np.int64)
    lone = np.asarray([np.abs(starts - int(x)).min() > 1_000_000 for x in rg["loc"]])
    assert sum(int(per[off[i]:off[i + 1]].sum()) > 0 for i in np.flatnonzero(lone)) > 5
    bad, nonzero, lone_nonzero = [], 0, 0
    groups = S.width_groups(rg)
    for w, idx in groups.items():
        part = S.take(rg, idx)
        want2 = A.want_coverage(data["cols"], part, 1, False, **kw)
        assert np.array_equal(want2, np.stack([per[off[i]:off[i + 1]] for i in idx]).astype(np.int64).sum(axis=0))
        want50 = A.want_coverage(data["cols"], part, 50, True, **kw)
        nonzero += bool(want2.any()) and bool(want50[1].any())
        # the ranges megabases from every cluster (template spans alone), summed
        if lone[idx].sum() >= 1:
            lone_nonzero += bool(A.want_coverage(data["cols"], S.take(rg, idx[lone[idx]]), 1, False, **kw).any())
        for form, got, _, _ in _extreme_forms(data, part, "cov2", 1, False, kw):
            _compare(bad, dict(kw, kind="cov2", w=w), form, got, want2, False)
        for form, got, _, _ in _extreme_forms(data, part, "covex", 50, True, kw):
            _compare(bad, dict(kw, kind="covex", binsize=50, w=w), form, got, want50, True)
    assert nonzero >= 4 and lone_nonzero >= 4, (nonzero, lone_nonzero)
    assert not bad, _summary(bad)
