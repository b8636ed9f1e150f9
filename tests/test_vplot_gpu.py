"""GPU: the V-plot over ranges of one width (bsig_plan_create_vplot, k_vplot_tiles; bamVPlot) against the definition -- one
bamProfile of the C oracle per row band, summed over the ranges (tests/vplot_expected.py).  All exact, in both forms of the
kernel: the table in LDS and global atomics (BAMSIGNALS_VPLOT_FORM=global).

The refusal of a tile with 2^32 reads in its windows is not exercised: no input a test can hold has one."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import vplot_expected as ve
from test_vplot_cpu import PARAM_RULE

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [2_000_000, 700_017]
LDS_COUNTERS = 40960                    # the budget B: the 160 KiB a gfx950 workgroup may declare, in 32-bit counters
PAIRS = (((0, 1000), 7), ((150, 300), 1), ((120, 5000), 64), ((0, 999), 1000))
FORMS = ("auto", "global", "auto+merge", "global+merge")        # (+merge: BAMSIGNALS_VPLOT_MERGE=1, not the default)


def _upload(ctx, cols):
    from bamsignals_amd.device import Reads
    if "cigar" in cols:
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                     cigar_off=cols["cigar_off"], cigar=cols["cigar"])
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])


@pytest.fixture(scope="module")
def synth():
    """paired reads on two references (the fragsizes fixture's recipe), resident on GPU 0, and the oracle's copy of them"""
    from bamsignals_amd.device import Context
    from bamsignals_amd.synth import synth_reads
    from oracle import oracle_c
    ctx = Context(0)
    cols = synth_reads(400_000, REF_LEN, seed=92, paired=True)
    cols["end"] = oracle_c.cigar_end(cols["pos"], cols["flag"], cols["cigar_off"], cols["cigar"])
    reads = _upload(ctx, cols)
    yield ctx, cols, reads, ve.oracle_reads(cols)
    reads.close()
    ctx.close()


def _params(tf, midpoint=True, binsize=1, **kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    kw.setdefault("requiredF", 66)
    return make_params(_lib.MODE_PROFILE, tlen_filter=tf, pe_mid=midpoint, binsize=binsize, **kw)


def _force(monkeypatch, form):
    if form.startswith("global"):
        monkeypatch.setenv("BAMSIGNALS_VPLOT_FORM", "global")
    else:
        monkeypatch.delenv("BAMSIGNALS_VPLOT_FORM", raising=False)
    if form.endswith("+merge"):
        monkeypatch.setenv("BAMSIGNALS_VPLOT_MERGE", "1")
    else:
        monkeypatch.delenv("BAMSIGNALS_VPLOT_MERGE", raising=False)


def _run(ctx, reads, rg, tf, lenbin, binsize, midpoint, form=None, runs=2, **kw):
    """a plan's first run (fused lookups) and its later ones (windows kept), which must agree; form: the form the plan
    must have chosen (None: whichever); (table, stats, runs, form)"""
    from bamsignals_amd.device import VplotPlan
    plan = VplotPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(tf, midpoint, binsize, **kw), lenbin)
    try:
        rows, cols = ve.shape(rg, tf, lenbin, binsize)
        assert (plan.rows, plan.cols, plan.cells) == (rows, cols, rows * cols)
        if form is not None and plan.cells:
            assert plan.form == (1 if form.startswith("global") or plan.cells > LDS_COUNTERS else 0), (form, plan.form, plan.cells)
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int64 and got[0].shape == (rows, cols)
        return got[0], plan.stats(), plan.runs, plan.form
    finally:
        plan.close()


def _oracle_kw(kw):
    return {k: v for k, v in kw.items() if k in ("mapqual", "filteredF")}


def _check(ctx, reads, orc, rg, tf, lenbin, binsize, midpoint, monkeypatch, forms=FORMS, runs=2, want=None, **kw):
    """both forms against the definition; the table"""
    if want is None:
        want = ve.expected(orc, rg, tf, lenbin, binsize, midpoint, **_oracle_kw(kw))
    for form in forms:
        _force(monkeypatch, form)
        got, st, _, _ = _run(ctx, reads, rg, tf, lenbin, binsize, midpoint, form=form, runs=runs, **kw)
        assert np.array_equal(got, want), (tf, lenbin, binsize, midpoint, form, kw, np.argwhere(got != want)[:8])
        assert st["cells"] == want.size and st["heavy_tiles"] == 0
    _force(monkeypatch, "auto")
    return want


def _ranges(n, w, seed, jitter=0):
    from bamsignals_amd.synth import synth_ranges
    return synth_ranges(n, w, REF_LEN, seed=seed, jitter=jitter)


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"tf{p[0][0]}-{p[0][1]}by{p[1]}")
@pytest.mark.parametrize("midpoint", [False, True])
@pytest.mark.parametrize("w", [1, 100, 2048, 2049, 2 * 16384 + 100])
def test_grid(synth, w, midpoint, pair, monkeypatch):
    ctx, cols, reads, orc = synth
    rg = _ranges(60 if w < 10_000 else 12, w, seed=w)
    assert len(set(rg["strand"].tolist())) == 3          # '+', '-' and '*'
    tf, lenbin = pair
    total = 0
    for binsize in sorted({1, 7, 50, w, w + 1}):
        total += int(_check(ctx, reads, orc, rg, tf, lenbin, binsize, midpoint, monkeypatch).sum())
    assert w < 2048 or total > 0                         # (not vacuous)


def test_marginals_on_the_gpu(synth, monkeypatch):
    """column sums = the SumPlan's result, row sums = the FragPlan's, on the same reads, ranges and parameters"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, SumPlan, make_params
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 2049, seed=2049)
    a = (rg["rid"], rg["loc"], rg["len"], rg["strand"])
    for midpoint in (False, True):
        for (tf, lenbin), binsize in zip(PAIRS, (1, 7, 50, 2050)):
            sp = SumPlan(ctx, reads, *a, _params(tf, midpoint, binsize))
            fp = FragPlan(ctx, reads, *a, make_params(_lib.MODE_COUNT, tlen_filter=tf, pe_mid=midpoint, binsize=-1, requiredF=66), lenbin)
            col_sums, row_sums = sp.run_host().copy(), fp.run_host().copy()
            sp.close()
            fp.close()
            for form in FORMS:
                _force(monkeypatch, form)
                got, _, _, _ = _run(ctx, reads, rg, tf, lenbin, binsize, midpoint, form=form, runs=1)
                assert np.array_equal(got.sum(axis=0), col_sums) and np.array_equal(got.sum(axis=1), row_sums)
                assert got.sum() > 0


def test_stats_are_a_count_plans(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 2048, seed=2048)
    got, st, _, _ = _run(ctx, reads, rg, (0, 1000), 7, 50, True, runs=1)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"],
                make_params(_lib.MODE_COUNT, tlen_filter=(0, 1000), pe_mid=True, binsize=-1, requiredF=66))
    cs = plan.stats()
    plan.close()
    assert st["cells"] == 143 * 41 and st["heavy_tiles"] == 0 and st["n_ranges"] == 60
    for k in ("visits", "visits_packed", "visits_short", "bytes_per_visit_packed", "bytes_per_visit_short", "bytes_per_visit_long"):
        assert st[k] == cs[k], k
    assert st["bytes_per_visit_packed"] == 8 and st["visits"] > 0


# ---- the form boundary -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf,lenbin,w,cells,form", [((0, 319), 2, 256, LDS_COUNTERS, 0), ((0, 999), 1000, 40_961, LDS_COUNTERS + 1, 1),
                                                    ((0, 255), 2, 319, LDS_COUNTERS - 128, 0)])
def test_form_boundary(synth, tf, lenbin, w, cells, form, monkeypatch):
    """B = 40,960 counters: a table of exactly B cells lives in LDS (its filter table then stays in global memory; 128
    cells fewer and the filter table just fits behind it), one of B + 1 (a prime: one row of 40,961 columns) takes the
    global form; all are the oracle's"""
    ctx, cols, reads, orc = synth
    rows = tf[1] // lenbin + 1
    assert rows * w == cells
    rg = _ranges(200 if w < 1000 else 40, w, seed=rows)
    for midpoint in (False, True):
        _force(monkeypatch, "auto")
        want = ve.expected(orc, rg, tf, lenbin, 1, midpoint)
        got, _, _, chose = _run(ctx, reads, rg, tf, lenbin, 1, midpoint)
        assert chose == form and got.shape == (rows, w)
        assert np.array_equal(got, want) and want.sum() > 0
        _check(ctx, reads, orc, rg, tf, lenbin, 1, midpoint, monkeypatch, forms=("global", "auto+merge"), runs=1, want=want)


# ---- seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,w", [(64, 64 * 3 + 17), (0, 16384 * 2 + 100)])
def test_seams(synth, tile, w, monkeypatch):
    """single fragments whose 5' end or midpoint lies on the first and last base of the range, of its tiles and of its
    bins, and one base outside each: forward and reverse reads, tlen of either sign, odd and even lengths, lengths around
    the filter's ends and a row's seam; '+' and '-' ranges, both forms"""
    ctx = synth[0]
    tf, lenbin, loc = (100, 301), 7, 40_000
    step = tile or 16384
    seams = [x for k in range(1, (w + step - 1) // step) for x in (k * step - 1, k * step)]     # every tile's last and first base
    assert len(seams) == 2 * ((w + step - 1) // step - 1) and (tile == 0 or seams[-2:] == [191, 192])
    xs = [-1, 0, 6, 7] + seams + [w - 8, w - 7, w - 1, w]
    inside = len(xs) - 2
    lengths = [99, 100, 301, 302, 139, 140, 146, 147, 200, 201]      # tf0 - 1, tf0, tf1, tf1 + 1, 20 * 7 - 1, 20 * 7, ..., even, odd
    parts = []
    for x in xs:
        t = loc + x
        for L in lengths:
            h = L // 2
            for neg_tlen in (False, True):
                parts.append(ve.planted(1, L, t, negative_tlen=neg_tlen))                      # forward, 5' end on t
                parts.append(ve.planted(2, L, t - h, negative_tlen=neg_tlen))                  # forward, midpoint on t (twice)
                parts.append(ve.planted(1, L, t, reverse=True, negative_tlen=neg_tlen))        # reverse: its 5' end is `end`
                parts.append(ve.planted(2, L, t + h, reverse=True, negative_tlen=neg_tlen))    # reverse, midpoint on t (twice)
    cols = ve.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        for binsize in (7, 1):
            tables = {}
            for strand in (1, -1):
                rg = dict(rid=[0], loc=[loc], len=[w], strand=[strand])
                for m in (False, True):
                    want = ve.expected(cols, rg, tf, lenbin, binsize, m)
                    # (the planting took: the positions inside, six lengths in the filter, both signs, two reads per rule)
                    assert want.sum() >= inside * 6 * 2 * 2 and want[:14].sum() == 0
                    assert want[:, 0].sum() > 0 and want[:, -1].sum() > 0
                    for form in FORMS:
                        _force(monkeypatch, form)
                        for threads in (64, 256):
                            got, st, _, _ = _run(ctx, reads, rg, tf, lenbin, binsize, m, form=form, tile_cells=tile, threads=threads)
                            assert np.array_equal(got, want), (binsize, strand, m, form, threads)
                            assert st["n_items"] == (w + step - 1) // step
                    tables[strand, m] = want
            for m in (False, True):
                assert not np.array_equal(tables[1, m], tables[-1, m])
                if w % binsize == 0:                     # (whole bins mirror onto whole bins)
                    assert np.array_equal(tables[1, m], tables[-1, m][:, ::-1])
            assert not np.array_equal(tables[1, False], tables[1, True])
    finally:
        reads.close()


def test_megabase_lengths(synth, monkeypatch):
    """template lengths of megabases under the midpoint rule: the reach of the windows, the full-width divisions, no
    24-bit arithmetic on a length, on half of one or on a position in the range"""
    ctx = synth[0]
    ref = 64_000_000
    tf, lenbin, binsize = (0, 20_000_000), 5000, 100
    big = [4_194_303, 4_194_304, 5_000_001, 19_999_999]
    parts, mids = [], []
    for k, L in enumerate(big):
        p = 1_000_000 + 3_000_017 * k
        parts.append(ve.planted(1 + k, L, p))                               # forward: midpoint p + L // 2
        parts.append(ve.planted(2, L, p + L - 1 + 5000, reverse=True))      # reverse: midpoint end - L // 2
        mids += [p + L // 2, p + L - 1 + 5000 - L // 2]
    rng = np.random.default_rng(7)
    n_bg = 3000
    bg_pos = rng.integers(0, ref - 25_000_000, n_bg)
    bg = dict(rid=np.zeros(n_bg, np.int64), pos=bg_pos, end=bg_pos + 49, flag=np.where(rng.random(n_bg) < 0.5, 99, 163),
              mapq=np.full(n_bg, 40), tlen=rng.integers(50, 21_000_000, n_bg))
    cols = ve.merge_sorted(parts + [bg], 1)
    cols["ref_len"] = np.asarray([ref], np.int64)
    reads = _upload(ctx, cols)
    try:
        mids = np.asarray(mids, np.int64)
        rg = dict(rid=np.zeros(len(mids), np.int32), loc=(mids - 700).astype(np.int32), len=np.full(len(mids), 1500, np.int32),
                  strand=np.resize([1, -1, 0], len(mids)).astype(np.int32))
        want = ve.expected(cols, rg, tf, lenbin, binsize, True)
        assert want.shape == (4001, 15) and want.size == 60_015
        for k, L in enumerate(big):
            r = L // lenbin
            band = (r * lenbin, min(tf[1], (r + 1) * lenbin - 1))
            assert np.array_equal(want[r], ve.profile_marginal(cols, rg, band, binsize, True))
            assert want[r].sum() >= 1 + k + 2
        _check(ctx, reads, cols, rg, tf, lenbin, binsize, True, monkeypatch, want=want)
    finally:
        reads.close()


# ---- piles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frag", [65_535, 65_536, 65_537])
@pytest.mark.parametrize("beside", [False, True])
def test_piles_on_one_base(synth, n_frag, beside, monkeypatch):
    """n fragments of one length on one base: every lane of a wave on one cell, and counts past 16 and 21 bits"""
    ctx = synth[0]
    at, L = 50_000, 167
    parts = [ve.planted(n_frag, L, at)]
    if beside:
        rng = np.random.default_rng(n_frag)
        p = rng.integers(45_000, 56_000, 3000)
        parts.append(dict(rid=np.zeros(3000, np.int64), pos=p, end=p + 49, flag=np.where(rng.random(3000) < 0.5, 99, 83),
                          mapq=np.full(3000, 30), tlen=rng.integers(90, 260, 3000) * np.where(rng.random(3000) < 0.5, -1, 1)))
    cols = ve.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    orc = ve.oracle_reads(cols)
    reads = _upload(ctx, cols)
    tf, lenbin, binsize = (100, 250), 10, 50
    try:
        for times in (1, 3, 40):
            rg = dict(rid=np.zeros(times, np.int32), loc=np.full(times, 49_000, np.int32), len=np.full(times, 3000, np.int32),
                      strand=np.ones(times, np.int32))
            for midpoint in (False, True):
                want = ve.expected(orc, rg, tf, lenbin, binsize, midpoint)
                assert want[L // lenbin].max() >= times * n_frag and (not beside or np.count_nonzero(want) > 100)
                for per in ("1", "1000000"):
                    monkeypatch.setenv("BAMSIGNALS_VPLOT_RUN_TILES", per)
                    _check(ctx, reads, orc, rg, tf, lenbin, binsize, midpoint, monkeypatch, runs=1 if times == 3 else 2, want=want)
        assert want.max() >= 40 * 65_535 > 2 ** 21
    finally:
        reads.close()


def test_run_lengths_and_the_lowered_ceiling(synth, monkeypatch):
    """one tile per workgroup, all tiles in one, and runs cut by the reads in their windows (LDS form)"""
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 2048, seed=2048)
    tf, lenbin, binsize = (0, 1000), 7, 50
    want = ve.expected(orc, rg, tf, lenbin, binsize, True)
    assert want.sum() > 5000
    for form in FORMS:
        _force(monkeypatch, form)
        counts = {}
        for per in ("1", "1000000", None):
            if per:
                monkeypatch.setenv("BAMSIGNALS_VPLOT_RUN_TILES", per)
            else:
                monkeypatch.delenv("BAMSIGNALS_VPLOT_RUN_TILES")
            got, st, counts[per], _ = _run(ctx, reads, rg, tf, lenbin, binsize, True, form=form)
            assert np.array_equal(got, want), (form, per)
        assert counts["1"] == st["n_items"] == 60 and counts["1000000"] == 1
        # every tile of these sees some 400 reads: a ceiling of 1,000 ends a run of the LDS form after two tiles; the
        # global form has no counter to protect
        monkeypatch.setenv("BAMSIGNALS_VPLOT_RUN_TILES", "1000000")
        monkeypatch.setenv("BAMSIGNALS_VPLOT_FLUSH_READS", "1000")
        got, st, cut, _ = _run(ctx, reads, rg, tf, lenbin, binsize, True, form=form)
        assert np.array_equal(got, want)
        if form.startswith("global"):
            assert cut == 1
        else:
            assert st["visits"] > 10_000 and 60 >= cut >= st["visits"] // 1000 > 1
        monkeypatch.delenv("BAMSIGNALS_VPLOT_FLUSH_READS")
        monkeypatch.delenv("BAMSIGNALS_VPLOT_RUN_TILES")


def test_filters_and_threads(synth, monkeypatch):
    ctx, cols, reads, orc = synth
    rg = _ranges(40, 3000, seed=5)
    for kw in (dict(filteredF=1024), dict(mapqual=30), dict(mapqual=30, filteredF=1024)):
        a = _check(ctx, reads, orc, rg, (0, 1000), 7, 50, True, monkeypatch, **kw)
        b = _check(ctx, reads, orc, rg, (100, 400), 1, 7, False, monkeypatch, runs=1, **kw)
        assert a.sum() > 0 and b.sum() > 0
    for threads in (64, 128, 256):
        for midpoint in (False, True):
            _check(ctx, reads, orc, rg, (0, 1000), 7, 25, midpoint, monkeypatch, threads=threads)


@pytest.mark.parametrize("env", [{}, {"BAMSIGNALS_PACKED_HALF": "0"}, {"BAMSIGNALS_PACK": "0"}])
def test_packed_forms(synth, env, monkeypatch):
    ctx, cols, _, orc = synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads = _upload(ctx, cols)
    try:
        rg = _ranges(80, 2500, seed=11)
        for midpoint in (False, True):
            want = _check(ctx, reads, orc, rg, (0, 1000), 7, 50, midpoint, monkeypatch)
            assert want.sum() > 0
        _, st, _, _ = _run(ctx, reads, rg, (0, 1000), 7, 50, True, runs=1)
        if env.get("BAMSIGNALS_PACK") == "0":
            assert st["visits_packed"] == 0
        else:
            assert st["visits_packed"] > 0 and st["bytes_per_visit_packed"] == 8      # the word and its tlen
    finally:
        reads.close()


def test_edges(synth, monkeypatch):
    ctx, cols, reads, orc = synth
    for form in FORMS:
        _force(monkeypatch, form)
        got, st, n_runs, _ = _run(ctx, reads, dict(rid=[], loc=[], len=[], strand=[]), (0, 500), 1, 1, False)
        assert got.shape == (501, 0) and st["n_items"] == 0 and n_runs == 0 and st["cells"] == 0
        got, st, _, _ = _run(ctx, reads, dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1]), (0, 700), 7, 3, True)
        assert got.shape == (101, 0)
    # an empty filter is a table of zeros, not an error
    want = _check(ctx, reads, orc, _ranges(20, 3000, seed=3), (300, 200), 1, 100, False, monkeypatch, runs=1)
    assert want.shape == (201, 30) and not want.any()


def test_caps(synth):
    from bamsignals_amd import _lib
    ctx, cols, reads, orc = synth
    for rg, tf, lenbin, binsize, says in (
            (_ranges(3, 3000, seed=77), (0, 16384), 1, 100, "tlen_filter[1] / len_bin + 1 = 16385 rows, at most 16384 fit: choose a wider len_bin"),
            (_ranges(3, 1025, seed=77), (0, 16383), 1, 1, "16384 rows x 1025 columns are more than 16777216 cells: choose a wider len_bin or binsize"),
            (_ranges(3, 33_556, seed=77), (0, 9999), 10, 2, "1000 rows x 16778 columns are more than 16777216 cells: choose a wider len_bin or binsize")):
        with pytest.raises(_lib.BsigError) as e:
            _run(ctx, reads, rg, tf, lenbin, binsize, True)
        assert (e.value.code_name, str(e.value)) == ("BSIG_ERR_ARG", says)
    # the widest table the caps allow: 16,384 rows x 1,024 columns, run once
    rg = _ranges(3, 1024, seed=78)
    got, _, _, form = _run(ctx, reads, rg, (0, 16383), 1, 1, True, runs=1)
    assert got.shape == (16384, 1024) and form == 1
    assert np.array_equal(got, ve.restated(cols, rg, (0, 16383), 1, 1, True)) and got.sum() > 0


# ---- plans -----------------------------------------------------------------------------------------------------------
def test_stale_plan_and_wrong_run_calls(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, HistPlan, Plan, ScaledPlan, SumPlan, SummaryPlan, VplotPlan, XcorrPlan, make_params
    ctx, cols, _, _ = synth
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        a = ([0], [10], [100], [1])
        prof = make_params(_lib.MODE_PROFILE)
        vp = VplotPlan(ctx, reads, *a, _params((0, 24)), 1)
        pp, sp, xp = Plan(ctx, reads, *a, prof), SumPlan(ctx, reads, *a, prof), XcorrPlan(ctx, reads, *a, prof, 20)
        fp = FragPlan(ctx, reads, *a, make_params(_lib.MODE_COUNT, tlen_filter=(0, 24), binsize=-1, requiredF=66), 1)
        hp, mp, cp = HistPlan(ctx, reads, *a, prof, 10), SummaryPlan(ctx, reads, *a, prof, (1, 5)), ScaledPlan(ctx, reads, *a, prof, 4)
        others = ((pp, ""), (sp, "_sum"), (xp, "_xcorr"), (fp, "_frag"), (hp, "_hist"), (mp, "_summary"), (cp, "_scaled"))
        b32, b64 = np.zeros(4000, np.int32), np.zeros(4000, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        cases = [(lib.bsig_plan_run_host, vp, p32, "a vplot plan runs with bsig_plan_run_vplot_host"),
                 (lib.bsig_plan_run, vp, p32, "a vplot plan runs with bsig_plan_run_vplot"),
                 (lib.bsig_plan_run_host_async, vp, p32, "a vplot plan runs with bsig_plan_run_vplot")]
        for kind in ("sum", "xcorr", "frag", "hist", "summary", "scaled"):
            cases.append((getattr(lib, f"bsig_plan_run_{kind}_host"), vp, p64, "a vplot plan runs with bsig_plan_run_vplot_host"))
            cases.append((getattr(lib, f"bsig_plan_run_{kind}"), vp, p64, "a vplot plan runs with bsig_plan_run_vplot"))
        for other, kind in others:
            cases.append((lib.bsig_plan_run_vplot_host, other, p64, f"not a vplot plan: bsig_plan_run{kind}_host runs it"))
            cases.append((lib.bsig_plan_run_vplot, other, p64, f"not a vplot plan: bsig_plan_run{kind} runs it"))
        for fn, plan, buf, says in cases:
            assert fn(plan._h, buf) == -1
            assert lib.bsig_last_error().decode() == says
        assert not b32.any() and not b64.any()
        for other, _ in others:
            for q in ("cells", "runs", "rows", "cols", "form"):
                assert getattr(lib, f"bsig_plan_vplot_{q}")(other._h) == 0
        assert lib.bsig_plan_vplot_cells(vp._h) == 25 * 100 and lib.bsig_plan_vplot_cells(None) == 0
        assert (lib.bsig_plan_vplot_rows(vp._h), lib.bsig_plan_vplot_cols(vp._h)) == (25, 100)
        for kind in ("sum", "xcorr", "frag", "hist", "summary", "scaled"):
            assert getattr(lib, f"bsig_plan_{kind}_cells")(vp._h) == 0
        first = vp.run_host()
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        with pytest.raises(_lib.BsigError, match="make a new plan"):
            vp.run_host()
        vp2 = VplotPlan(ctx, reads, *a, _params((0, 24)), 1)
        assert np.array_equal(vp2.run_host(), first)
        for p in (vp, vp2) + tuple(o for o, _ in others):
            p.close()
    finally:
        reads.close()


def test_errors(synth):
    """the parameter rule's table (tests/test_vplot_cpu.py) and what only the plan call can express"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import VplotPlan, make_params
    ctx, cols, reads, _ = synth
    for kw, code, message in PARAM_RULE:
        kw = dict(kw)
        tf = kw.get("tlen_filter", (0, 1000))
        width = kw.get("width", (100, 100))
        p = _lib.Params()
        p.mode, p.binsize, p.filteredF, p.requiredF, p.pe_mid = _lib.MODE_PROFILE, kw.get("binsize", 1), -1, 66, 1
        p.n_tlen_filter = len(tf)
        for i, v in enumerate(tf):
            p.tlen_filter[i] = v
        with pytest.raises(_lib.BsigError) as e:
            VplotPlan(ctx, reads, [0, 1], [999, 999], list(width), [1, 1], p, kw.get("len_bin", 1))
        assert (e.value.code, str(e.value)) == (code, message)
    a = ([0], [10], [100], [1])
    for kw, message in ((dict(shift=1), "the V-plot counts unshifted positions: shift must be 0"),
                        (dict(ss=True), "the V-plot has no strand split: ss must be 0"), (dict(threads=96), "threads must be")):
        with pytest.raises(_lib.BsigError, match=message) as e:
            VplotPlan(ctx, reads, *a, _params((0, 100), **kw), 1)
        assert e.value.code_name == "BSIG_ERR_ARG"
    for mode in (_lib.MODE_COUNT, _lib.MODE_COVERAGE):
        with pytest.raises(_lib.BsigError, match="the V-plot is defined on bamProfile") as e:
            VplotPlan(ctx, reads, *a, make_params(mode, tlen_filter=(0, 100), requiredF=66), 1)
        assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError, match="must not be negative") as e:
        VplotPlan(ctx, reads, *a, _params((-5, -1)), 1)
    assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError) as e:
        VplotPlan(ctx, reads, [5], [10], [100], [1], _params((0, 100)), 1)
    assert e.value.code_name == "BSIG_ERR_CHROM"


# ---- file level ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(fixture_reads):
    from bamsignals_amd import GRanges
    fx = fixture_reads
    names = [str(s) for s in fx["ref_names"]]
    rng = np.random.default_rng(31)
    n, w = 50, 1500
    rid = rng.integers(0, len(names), n).astype(np.int32)
    loc = np.asarray([rng.integers(0, max(int(fx["ref_len"][r]) - w, 1)) for r in rid], np.int32)
    strand = np.asarray([1, -1, 0], np.int32)[rng.integers(0, 3, n)]
    assert len(set(strand.tolist())) == 3
    gr = GRanges([names[r] for r in rid], loc + 1, width=np.full(n, w, np.int32), strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in strand])
    rg = dict(rid=rid, loc=loc, len=np.full(n, w, np.int32), strand=strand)
    cols = dict(ref_off=fx["ref_off"], pos=fx["bam_pos"], end=fx["bam_end"], flag=fx["bam_flag"], mapq=fx["bam_mapq"],
                tlen=fx["bam_tlen"])
    return gr, rg, cols


@pytest.fixture(params=["all", "regions"])
def decode_mode(request, monkeypatch):
    from bamsignals_amd import _lib
    monkeypatch.setenv("BAMSIGNALS_DECODE", request.param)
    _lib.load().bsig_cache_clear()
    yield request.param
    _lib.load().bsig_cache_clear()


def test_file_level(fixture, decode_mode):
    from bamsignals_amd import VPlot, bamFragSizes, bamProfile, bamVPlot
    from bamsignals_amd.wrappers import tlenFilter
    gr, rg, cols = fixture
    orc = ve.oracle_reads(cols)
    for pe in ("filter", "midpoint"):
        for tf in (None, (50, 300)):
            for lenbin, binsize in ((1, 1), (10, 25), (1, 25), (10, 1)):
                vp = bamVPlot(BAM, gr, tlenFilter=tf, lenbin=lenbin, binsize=binsize, paired_end=pe, verbose=False)
                want = ve.expected(orc, rg, tlenFilter(tf, pe), lenbin, binsize, pe == "midpoint")
                assert isinstance(vp, VPlot) and vp.counts.dtype == np.int64 and vp.counts.shape == want.shape
                assert np.array_equal(vp.counts, want), (pe, tf, lenbin, binsize)
                assert vp.n == int(want.sum()) > 0 and (vp.lenbin, vp.binsize) == (lenbin, binsize)
                fs = bamFragSizes(BAM, gr, tlenFilter=tf, lenbin=lenbin, paired_end=pe, verbose=False)
                assert np.array_equal(vp.frag_sizes().counts, fs.counts)
                prof = bamProfile(BAM, gr, binsize=binsize, paired_end=pe, tlenFilter=tf, aggregate=True, verbose=False)
                assert np.array_equal(vp.profile(), prof)
    vp = bamVPlot(BAM, gr, lenbin=10, binsize=25, mapqual=30, filteredFlag=1024, verbose=False)
    assert np.array_equal(vp.counts, ve.expected(orc, rg, (0, 1000), 10, 25, True, mapqual=30, filteredF=1024))


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import bamVPlot
    from bamsignals_amd.wrappers import last_call_route
    from bamsignals_amd import _lib
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
        one = bamVPlot(BAM, gr, lenbin=3, binsize=10, verbose=False)
        assert "1 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
        four = bamVPlot(BAM, gr, lenbin=3, binsize=10, verbose=False)
        assert "4 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
        assert np.array_equal(one.counts, four.counts) and one.counts.any() and one.n == four.n
    finally:
        _lib.load().bsig_cache_clear()


# ---- the use ---------------------------------------------------------------------------------------------------------
def test_the_v_is_read_off_the_data(synth, tmp_path):
    """20,000 fragments of 120 bp centred on 200 sites and 20,000 of 190 bp centred 150 bp to either side, over the
    synthetic background: the short band peaks on the site, the long band at +-150"""
    from bamsignals_amd import GRanges, bamVPlot, write_columns_as_bam
    from bamsignals_amd import _lib
    ctx, bg, _, _ = synth
    ref_off = np.asarray(bg["ref_off"])
    rng = np.random.default_rng(120)
    sites = np.sort(rng.choice(np.arange(2000, REF_LEN[0] - 2000, 2500), 200, replace=False)).astype(np.int64)
    centre = np.repeat(sites, 100)
    side = centre + np.where(rng.random(len(centre)) < 0.5, -150, 150)
    half = len(centre) // 2
    parts = [dict(rid=np.repeat(np.arange(2), np.diff(ref_off)), pos=bg["pos"], end=bg["end"], flag=bg["flag"], mapq=bg["mapq"],
                  tlen=bg["tlen"]),
             ve.planted(half, 120, centre[:half] - 60), ve.planted(half, 120, centre[half:] + 60, reverse=True),
             ve.planted(half, 190, side[:half] - 95), ve.planted(half, 190, side[half:] + 95, reverse=True)]
    cols = ve.merge_sorted(parts, 2)
    cols["ref_len"] = np.asarray(REF_LEN, np.int64)
    w = 1001
    rg = dict(rid=np.zeros(200, np.int32), loc=(sites - 500).astype(np.int32), len=np.full(200, w, np.int32), strand=np.ones(200, np.int32))
    tf, lenbin = (0, 399), 20

    def says_v(vp):
        short, long_ = vp.band(100, 139), vp.band(180, 199)
        assert int(np.argmax(short)) == 500 and short[500] >= 20_000
        top = set(np.argsort(long_)[-2:].tolist())
        assert top == {350, 650} and long_[350] + long_[650] >= 20_000

    from bamsignals_amd import VPlot
    want = ve.expected(cols, rg, tf, lenbin, 1, True)
    says_v(VPlot(want, lenbin, 1))                         # the definition says so first
    bam = str(tmp_path / "v.bam")
    cig = dict(cigar_off=np.arange(len(cols["pos"]) + 1, dtype=np.int64),
               cigar=((cols["end"].astype(np.int64) - cols["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(bam, ["chrA", "chrB"], dict(cols, **cig))
    try:
        vp = bamVPlot(bam, GRanges(["chrA"] * 200, sites - 500 + 1, width=np.full(200, w), strand=["+"] * 200), tlenFilter=tf,
                      lenbin=lenbin, verbose=False)
        assert np.array_equal(vp.counts, want)
        says_v(vp)
    finally:
        _lib.load().bsig_cache_clear()
