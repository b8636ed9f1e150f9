"""GPU: the fragment-length histogram over ranges (bsig_plan_create_frag, k_frag_tiles; bamFragSizes) against the
definition -- one bamCount of the C oracle per row, summed over the ranges (tests/fragsizes_expected.py).  All exact.

The refusal of a tile with 2^32 reads in its windows is not exercised: no input a test can hold has one."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import fragsizes_expected as fe
from test_fragsizes_cpu import PARAM_RULE

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [2_000_000, 700_017]
CAP = 16384
PAIRS = (((0, 1000), 1), ((0, 1000), 7), ((150, 300), 1), ((0, 999), 1000), ((120, 5000), 64))


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
    yield ctx, cols, reads, fe.oracle_reads(cols)
    reads.close()
    ctx.close()


def _params(tf, midpoint=False, **kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    kw.setdefault("requiredF", 66)
    return make_params(_lib.MODE_COUNT, tlen_filter=tf, pe_mid=midpoint, binsize=-1, **kw)


def _run(ctx, reads, rg, tf, lenbin, midpoint, runs=2, **kw):
    """a plan's first run (fused lookups) and its later ones (windows kept), which must agree; (result, stats, runs)"""
    from bamsignals_amd.device import FragPlan
    plan = FragPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(tf, midpoint, **kw), lenbin)
    try:
        assert plan.cells == tf[1] // lenbin + 1
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int64 and got[0].shape == (plan.cells,)
        return got[0], plan.stats(), plan.runs
    finally:
        plan.close()


def _oracle_kw(kw):
    return {k: v for k, v in kw.items() if k in ("mapqual", "filteredF")}


def _check(ctx, reads, orc, rg, tf, lenbin, midpoint, runs=2, **kw):
    got, st, n_runs = _run(ctx, reads, rg, tf, lenbin, midpoint, runs=runs, **kw)
    want = fe.expected(orc, rg, tf, lenbin, midpoint, **_oracle_kw(kw))
    assert np.array_equal(got, want), (tf, lenbin, midpoint, kw, np.flatnonzero(got != want)[:8])
    assert st["cells"] == len(want) and st["heavy_tiles"] == 0
    return got, st, n_runs


def _ranges(n, w, seed, jitter=0):
    from bamsignals_amd.synth import synth_ranges
    return synth_ranges(n, w, REF_LEN, seed=seed, jitter=jitter)


def _cat(*rgs):
    return {k: np.concatenate([np.asarray(r[k], np.int32) for r in rgs]) for k in ("rid", "loc", "len", "strand")}


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("midpoint", [False, True])
@pytest.mark.parametrize("w", [1, 100, 2048, 2049, 10_000])
def test_grid(synth, w, midpoint):
    ctx, cols, reads, orc = synth
    rg = _ranges(60 if w < 10_000 else 12, w, seed=w)
    assert w >= 10_000 or len(set(rg["strand"].tolist())) == 3
    total = 0
    for tf, lenbin in PAIRS:
        got, st, _ = _check(ctx, reads, orc, rg, tf, lenbin, midpoint)
        total += int(got.sum())
    assert w < 2048 or total > 5000                      # (not vacuous)


def test_stats_are_a_count_plans(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 2048, seed=2048)
    got, st, _ = _run(ctx, reads, rg, (0, 1000), 7, True, runs=1)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"],
                make_params(_lib.MODE_COUNT, tlen_filter=(0, 1000), pe_mid=True, binsize=-1, requiredF=66))
    cs = plan.stats()
    plan.close()
    assert st["cells"] == 143 and st["heavy_tiles"] == 0 and st["n_ranges"] == 60
    for k in ("visits", "visits_packed", "visits_short", "bytes_per_visit_packed", "bytes_per_visit_short", "bytes_per_visit_long"):
        assert st[k] == cs[k], k
    assert st["bytes_per_visit_packed"] == 8 and st["visits"] > 0


def test_cap(synth):
    from bamsignals_amd import _lib
    ctx, cols, reads, orc = synth
    rg = _ranges(3, 3000, seed=77)
    got, _, _ = _check(ctx, reads, orc, rg, (0, CAP - 1), 1, True)
    assert len(got) == CAP and got.sum() > 0
    got, _, _ = _check(ctx, reads, orc, rg, (0, 10 * CAP - 1), 10, False, runs=1)
    assert len(got) == CAP and got.sum() > 0
    with pytest.raises(_lib.BsigError, match="16385 rows") as e:
        _run(ctx, reads, rg, (0, CAP), 1, False)
    assert e.value.code_name == "BSIG_ERR_ARG"


def test_whole_references_with_short_ranges_and_flipped_strands(synth):
    """both references whole, short ranges, zero widths, duplicates, overhangs on both ends: one call; the strand of a
    range does not matter"""
    ctx, cols, reads, orc = synth
    whole = dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[1, -1])
    short = _ranges(40, 300, seed=8, jitter=290)
    edge = dict(rid=[0, 0, 1, 1, 0, 0, 1], loc=[-700, 1_999_500, -3, 700_000, 5000, 5000, 40], len=[1500, 900, 10, 600, 0, 777, 0],
                strand=[1, -1, 0, 1, 1, -1, 0])
    rg = _cat(whole, short, edge, short, dict(rid=[0, 0], loc=[5000, 5000], len=[777, 777], strand=[-1, -1]))
    for midpoint in (False, True):
        got, _, _ = _check(ctx, reads, orc, rg, (0, 1000), 7, midpoint)
        assert got.sum() >= 199_984 - 400                # the whole references' fragments (but a midpoint past the end)
        flipped = dict(rg, strand=-np.asarray(rg["strand"]))
        for strands in (flipped, dict(rg, strand=np.zeros_like(rg["strand"]))):
            assert np.array_equal(_run(ctx, reads, strands, (0, 1000), 7, midpoint, runs=1)[0], got)


def test_edges(synth):
    ctx, cols, reads, orc = synth
    got, st, n_runs = _run(ctx, reads, dict(rid=[], loc=[], len=[], strand=[]), (0, 500), 1, False)
    assert got.shape == (501,) and not got.any() and st["n_items"] == 0 and n_runs == 0
    got, st, _ = _run(ctx, reads, dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1]), (0, 700), 7, True)
    assert got.shape == (101,) and not got.any()
    # an empty filter is a histogram of zeros, not an error
    got, _, _ = _check(ctx, reads, orc, _ranges(20, 3000, seed=3), (300, 200), 1, False, runs=1)
    assert got.shape == (201,) and not got.any()


def test_filters_and_threads(synth):
    ctx, cols, reads, orc = synth
    rg = _ranges(40, 3000, seed=5, jitter=800)
    for kw in (dict(filteredF=1024), dict(mapqual=30), dict(mapqual=30, filteredF=1024)):
        a, _, _ = _check(ctx, reads, orc, rg, (0, 1000), 7, True, **kw)
        b, _, _ = _check(ctx, reads, orc, rg, (100, 400), 1, False, runs=1, **kw)
        assert a.sum() > 0 and b.sum() > 0
    for threads in (64, 128, 256):
        for midpoint in (False, True):
            _check(ctx, reads, orc, rg, (0, 1000), 1, midpoint, threads=threads)


@pytest.mark.parametrize("env", [{}, {"BAMSIGNALS_PACKED_HALF": "0"}, {"BAMSIGNALS_PACK": "0"}])
def test_packed_forms(synth, env, monkeypatch):
    ctx, cols, _, orc = synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads = _upload(ctx, cols)
    try:
        for midpoint in (False, True):
            got, st, _ = _check(ctx, reads, orc, _ranges(80, 2500, seed=11), (0, 1000), 7, midpoint)
            assert got.sum() > 0
            if env.get("BAMSIGNALS_PACK") == "0":
                assert st["visits_packed"] == 0
            else:
                assert st["visits_packed"] > 0 and st["bytes_per_visit_packed"] == 8      # the word and its tlen
    finally:
        reads.close()


def test_run_lengths_and_the_lowered_ceiling(synth, monkeypatch):
    """one tile per workgroup, all tiles in one, and runs cut by the reads in their windows"""
    ctx, cols, reads, orc = synth
    rg = _ranges(60, 2048, seed=2048)
    tf, lenbin = (0, 1000), 7
    want = fe.expected(orc, rg, tf, lenbin, True)
    assert want.sum() > 5000
    for form in ("merge", "plain"):
        monkeypatch.setenv("BAMSIGNALS_FRAG_FORM", form)
        counts = {}
        for per in ("1", "1000000", None):
            if per:
                monkeypatch.setenv("BAMSIGNALS_FRAG_RUN_TILES", per)
            else:
                monkeypatch.delenv("BAMSIGNALS_FRAG_RUN_TILES")
            got, st, counts[per] = _run(ctx, reads, rg, tf, lenbin, True)
            assert np.array_equal(got, want), (form, per)
        assert counts["1"] == st["n_items"] == 60 and counts["1000000"] == 1
        # every tile of these sees some 400 reads: a ceiling of 1,000 ends a run after two tiles
        monkeypatch.setenv("BAMSIGNALS_FRAG_RUN_TILES", "1000000")
        monkeypatch.setenv("BAMSIGNALS_FRAG_FLUSH_READS", "1000")
        got, st, cut = _run(ctx, reads, rg, tf, lenbin, True)
        assert np.array_equal(got, want)
        assert st["visits"] > 10_000 and 60 >= cut >= st["visits"] // 1000 > 1
        monkeypatch.delenv("BAMSIGNALS_FRAG_FLUSH_READS")
        monkeypatch.delenv("BAMSIGNALS_FRAG_RUN_TILES")


# ---- seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,w", [(64, 64 * 3 + 17), (0, 16384 * 2 + 100)])
def test_seams(synth, tile, w):
    """single fragments whose 5' end or midpoint lies on the first and last base of the range and of its tiles, and one
    base outside: forward and reverse reads, tlen of either sign, lengths around the filter's ends and the rows' seams"""
    ctx = synth[0]
    tf, lenbin, loc = (100, 301), 7, 40_000
    step = tile or 16384
    xs = [-1, 0, step - 1, step, 2 * step - 1, 2 * step, w - 1, w]
    lengths = [99, 100, 301, 302, 139, 140, 146, 147, 200, 201]      # tf0 - 1, tf0, tf1, tf1 + 1, 20 * 7 - 1, 20 * 7, ..., even, odd
    parts = []
    for x in xs:
        t = loc + x
        for L in lengths:
            h = L // 2
            for neg_tlen in (False, True):
                parts.append(fe.planted(1, L, t, negative_tlen=neg_tlen))                      # forward, 5' end on t
                parts.append(fe.planted(2, L, t - h, negative_tlen=neg_tlen))                  # forward, midpoint on t (twice)
                parts.append(fe.planted(1, L, t, reverse=True, negative_tlen=neg_tlen))        # reverse: its 5' end is `end`
                parts.append(fe.planted(2, L, t + h, reverse=True, negative_tlen=neg_tlen))    # reverse, midpoint on t (twice)
    cols = fe.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=[0], loc=[loc], len=[w], strand=[1])
        wants = {m: fe.expected(cols, rg, tf, lenbin, m) for m in (False, True)}
        # (the planting took: six positions inside, six lengths in the filter, both signs, two reads per rule)
        for m in (False, True):
            assert wants[m].sum() >= 6 * 6 * 2 * 2 and wants[m][:14].sum() == 0
        assert not np.array_equal(wants[False], wants[True])
        # a forward read of length 301 whose midpoint is the range's first base lies wholly in front of the range
        assert fe.expected(fe.merge_sorted([fe.planted(1, 301, loc - 150)], 1), rg, tf, lenbin, True)[43] == 1
        for m in (False, True):
            for threads in (64, 256):
                got, st, _ = _run(ctx, reads, rg, tf, lenbin, m, tile_cells=tile, threads=threads)
                assert np.array_equal(got, wants[m]), (m, threads)
                assert st["n_items"] == (w + step - 1) // step
    finally:
        reads.close()


def test_megabase_lengths(synth):
    """template lengths of megabases under the midpoint rule: the reach of the windows, the full-width division, no
    24-bit arithmetic on a length or on half of one"""
    ctx = synth[0]
    ref = 64_000_000
    tf, lenbin = (0, 20_000_000), 2000
    big = [4_194_303, 4_194_304, 5_000_001, 19_999_999]
    parts, mids = [], []
    for k, L in enumerate(big):
        p = 1_000_000 + 3_000_017 * k
        parts.append(fe.planted(1 + k, L, p))                               # forward: midpoint p + L // 2
        parts.append(fe.planted(2, L, p + L - 1 + 5000, reverse=True))      # reverse: midpoint end - L // 2
        mids += [p + L // 2, p + L - 1 + 5000 - L // 2]
    rng = np.random.default_rng(7)
    n_bg = 3000
    bg_pos = rng.integers(0, ref - 25_000_000, n_bg)
    bg = dict(rid=np.zeros(n_bg, np.int64), pos=bg_pos, end=bg_pos + 49, flag=np.where(rng.random(n_bg) < 0.5, 99, 163),
              mapq=np.full(n_bg, 40), tlen=rng.integers(50, 21_000_000, n_bg))
    cols = fe.merge_sorted(parts + [bg], 1)
    cols["ref_len"] = np.asarray([ref], np.int64)
    reads = _upload(ctx, cols)
    try:
        mids = np.asarray(mids, np.int64)
        rg = dict(rid=np.zeros(len(mids) + 1, np.int32), loc=np.concatenate([mids - 700, [20_000_000]]).astype(np.int32),
                  len=np.concatenate([np.full(len(mids), 1500), [6_000_000]]).astype(np.int32),
                  strand=np.resize([1, -1, 0], len(mids) + 1).astype(np.int32))
        want = fe.expected(cols, rg, tf, lenbin, True)
        assert len(want) == 10_001
        for k, L in enumerate(big):
            assert want[L // lenbin] >= 1 + k + 2
        assert want.sum() > sum(3 + k for k in range(4)) + 50          # ... and background fragments beside them
        got, _, _ = _run(ctx, reads, rg, tf, lenbin, True)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        _check(ctx, reads, cols, rg, (4_194_304, 19_999_998), 4099, True, runs=1)
    finally:
        reads.close()


# ---- piles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frag", [65_535, 65_536, 65_537, 70_000])
@pytest.mark.parametrize("beside", [False, True])
def test_piles_on_one_base(synth, n_frag, beside, monkeypatch):
    """n fragments of one length on one base: every lane of a wave on one LDS cell, and counts past 16 bits"""
    ctx = synth[0]
    at, L = 50_000, 167
    parts = [fe.planted(n_frag, L, at)]
    if beside:
        rng = np.random.default_rng(n_frag)
        p = rng.integers(45_000, 56_000, 3000)
        parts.append(dict(rid=np.zeros(3000, np.int64), pos=p, end=p + 49, flag=np.where(rng.random(3000) < 0.5, 99, 83),
                          mapq=np.full(3000, 30), tlen=rng.integers(90, 260, 3000) * np.where(rng.random(3000) < 0.5, -1, 1)))
    cols = fe.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    orc = fe.oracle_reads(cols)
    reads = _upload(ctx, cols)
    tf, lenbin = (100, 250), 1
    try:
        for times in (1, 3, 40):
            rg = dict(rid=np.zeros(times, np.int32), loc=np.full(times, 49_000, np.int32), len=np.full(times, 3000, np.int32),
                      strand=np.resize([1, -1, 0], times).astype(np.int32))
            for midpoint in (False, True):
                want = fe.expected(orc, rg, tf, lenbin, midpoint)
                assert want[L] >= times * n_frag and (not beside or np.count_nonzero(want) > 100)
                for per, form in (("1", "merge"), ("1000000", "merge"), ("1", "plain"), ("1000000", "plain")):
                    monkeypatch.setenv("BAMSIGNALS_FRAG_RUN_TILES", per)
                    monkeypatch.setenv("BAMSIGNALS_FRAG_FORM", form)
                    got, st, _ = _run(ctx, reads, rg, tf, lenbin, midpoint, runs=1 if times == 3 else 2)
                    assert np.array_equal(got, want), (times, midpoint, per, form)
                    assert st["heavy_tiles"] == 0
        assert got[L] >= 40 * 65_535 > 2 ** 21
    finally:
        reads.close()


# ---- plans -----------------------------------------------------------------------------------------------------------
def test_stale_plan_and_wrong_run_calls(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, Plan, SumPlan, XcorrPlan, make_params
    ctx, cols, _, _ = synth
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        a = ([0], [10], [100], [1])
        prof = make_params(_lib.MODE_PROFILE)
        fp = FragPlan(ctx, reads, *a, _params((0, 24)), 1)
        pp, sp, xp = Plan(ctx, reads, *a, prof), SumPlan(ctx, reads, *a, prof), XcorrPlan(ctx, reads, *a, prof, 20)
        b32, b64 = np.zeros(400, np.int32), np.zeros(400, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        for fn, plan, buf, says in (
                (lib.bsig_plan_run_host, fp, p32, "a frag plan runs with bsig_plan_run_frag_host"),
                (lib.bsig_plan_run, fp, p32, "a frag plan runs with bsig_plan_run_frag"),
                (lib.bsig_plan_run_host_async, fp, p32, "a frag plan runs with bsig_plan_run_frag"),
                (lib.bsig_plan_run_sum_host, fp, p64, "a frag plan runs with bsig_plan_run_frag_host"),
                (lib.bsig_plan_run_sum, fp, p64, "a frag plan runs with bsig_plan_run_frag"),
                (lib.bsig_plan_run_xcorr_host, fp, p64, "a frag plan runs with bsig_plan_run_frag_host"),
                (lib.bsig_plan_run_xcorr, fp, p64, "a frag plan runs with bsig_plan_run_frag"),
                (lib.bsig_plan_run_frag_host, pp, p64, "not a frag plan: bsig_plan_run_host runs it"),
                (lib.bsig_plan_run_frag, pp, p64, "not a frag plan: bsig_plan_run runs it"),
                (lib.bsig_plan_run_frag_host, sp, p64, "not a frag plan: bsig_plan_run_sum_host runs it"),
                (lib.bsig_plan_run_frag, sp, p64, "not a frag plan: bsig_plan_run_sum runs it"),
                (lib.bsig_plan_run_frag_host, xp, p64, "not a frag plan: bsig_plan_run_xcorr_host runs it"),
                (lib.bsig_plan_run_frag, xp, p64, "not a frag plan: bsig_plan_run_xcorr runs it")):
            assert fn(plan._h, buf) == -1
            assert lib.bsig_last_error().decode() == says
        assert not b32.any() and not b64.any()
        for other in (pp, sp, xp):
            assert lib.bsig_plan_frag_cells(other._h) == 0 and lib.bsig_plan_frag_runs(other._h) == 0
        assert lib.bsig_plan_frag_cells(fp._h) == 25 and lib.bsig_plan_frag_cells(None) == 0
        assert lib.bsig_plan_xcorr_cells(fp._h) == 0 and lib.bsig_plan_sum_cells(fp._h) == 0
        first = fp.run_host()
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        with pytest.raises(_lib.BsigError, match="make a new plan"):
            fp.run_host()
        fp2 = FragPlan(ctx, reads, *a, _params((0, 24)), 1)
        assert np.array_equal(fp2.run_host(), first)
        for p in (fp, fp2, pp, sp, xp):
            p.close()
    finally:
        reads.close()


def test_errors(synth):
    """the parameter rule's table (tests/test_fragsizes_cpu.py) and what only the plan call can express"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, make_params
    ctx, cols, reads, _ = synth
    a = ([0], [10], [100], [1])
    for kw, code, message in PARAM_RULE:
        kw = dict(kw)
        tf = kw.get("tlen_filter", (0, 1000))
        p = _lib.Params()
        p.mode, p.binsize, p.filteredF, p.requiredF = _lib.MODE_COUNT, -1, -1, 66
        p.n_tlen_filter = len(tf)
        for i, v in enumerate(tf):
            p.tlen_filter[i] = v
        with pytest.raises(_lib.BsigError) as e:
            FragPlan(ctx, reads, *a, p, kw.get("len_bin", 1))
        assert (e.value.code, str(e.value)) == (code, message)
    for kw, message in ((dict(shift=1), "shift must be 0"), (dict(threads=96), "threads must be")):
        with pytest.raises(_lib.BsigError, match=message) as e:
            FragPlan(ctx, reads, *a, _params((0, 100), **kw), 1)
        assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError, match="defined on bamCount") as e:
        FragPlan(ctx, reads, *a, make_params(_lib.MODE_PROFILE, tlen_filter=(0, 100), requiredF=66), 1)
    assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError, match="must not be negative") as e:
        FragPlan(ctx, reads, *a, _params((-5, -1)), 1)
    assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError) as e:
        FragPlan(ctx, reads, [5], [10], [100], [1], _params((0, 100)), 1)
    assert e.value.code_name == "BSIG_ERR_CHROM"
    with pytest.raises(_lib.BsigError, match="negative width") as e:
        FragPlan(ctx, reads, [0], [10], [-1], [1], _params((0, 100)), 1)


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
    return gr, rg, cols


@pytest.fixture(params=["all", "regions"])
def decode_mode(request, monkeypatch):
    from bamsignals_amd import _lib
    monkeypatch.setenv("BAMSIGNALS_DECODE", request.param)
    _lib.load().bsig_cache_clear()
    yield request.param
    _lib.load().bsig_cache_clear()


def test_the_fixture_is_what_the_issue_says(fixture):
    gr, rg, cols = fixture
    flag, a = np.asarray(cols["flag"], np.int64), np.abs(np.asarray(cols["tlen"], np.int64))
    first = (flag & 66) == 66
    assert int(first.sum()) == 49_457 and (int(a[first].min()), int(a[first].max())) == (26, 400)


def test_file_level(fixture, decode_mode):
    from bamsignals_amd import bamCount, bamFragSizes
    from bamsignals_amd.wrappers import tlenFilter
    gr, rg, cols = fixture
    orc = fe.oracle_reads(cols)
    for pe in ("filter", "midpoint"):
        for tf in (None, (50, 300), (0, 400)):
            for lenbin in (1, 10):
                fs = bamFragSizes(BAM, gr, tlenFilter=tf, lenbin=lenbin, paired_end=pe, verbose=False)
                want = fe.expected(orc, rg, tlenFilter(tf, pe), lenbin, pe == "midpoint")
                assert np.array_equal(fs.counts, want) and fs.counts.dtype == np.int64, (pe, tf, lenbin)
                assert fs.n == int(want.sum()) > 0 and fs.lenbin == lenbin
                assert fs.n == int(np.asarray(bamCount(BAM, gr, paired_end=pe, tlenFilter=tf, verbose=False), np.int64).sum())
    fs = bamFragSizes(BAM, gr, mapqual=30, filteredFlag=1024, verbose=False)
    assert np.array_equal(fs.counts, fe.expected(orc, rg, (0, 1000), 1, False, mapqual=30, filteredF=1024))


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import bamFragSizes
    from bamsignals_amd.wrappers import last_call_route
    from bamsignals_amd import _lib
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
        one = bamFragSizes(BAM, gr, lenbin=3, paired_end="midpoint", verbose=False)
        assert "1 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
        four = bamFragSizes(BAM, gr, lenbin=3, paired_end="midpoint", verbose=False)
        assert "4 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
        assert np.array_equal(one.counts, four.counts) and one.counts.any() and one.n == four.n
    finally:
        _lib.load().bsig_cache_clear()


# ---- the use ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [147, 200, 431])
def test_fragment_length_is_read_off_the_data(synth, length, tmp_path):
    """20,000 fragments of one length over the synthetic background: mode() is that length.  The background's generator
    lifts every length below 100 to 100 (29,336 first reads of 199,984, more than are planted): tlenFilter starts at
    101, behind that artefact, so that the planted length is the oracle's unique maximum"""
    from bamsignals_amd import GRanges, bamFragSizes, write_columns_as_bam
    from bamsignals_amd import _lib
    ctx, bg, _, _ = synth
    ref_off = np.asarray(bg["ref_off"])
    rng = np.random.default_rng(length)
    at = rng.integers(0, REF_LEN[0] - 1000, 20_000)
    parts = [dict(rid=np.repeat(np.arange(2), np.diff(ref_off)), pos=bg["pos"], end=bg["end"], flag=bg["flag"], mapq=bg["mapq"],
                  tlen=bg["tlen"]),
             fe.planted(20_000, length, at)]
    cols = fe.merge_sorted(parts, 2)
    cols["ref_len"] = np.asarray(REF_LEN, np.int64)
    rg = dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[1, 0])
    tf = (101, 1000)
    assert fe.whole_count(cols, rg, (100, 100), False) > 20_000
    want = fe.expected(cols, rg, tf, 1, False)
    assert int(np.argmax(want)) == length and np.sum(want == want.max()) == 1      # the oracle's own maximum, unique
    bam = str(tmp_path / "frag.bam")
    cig = dict(cigar_off=np.arange(len(cols["pos"]) + 1, dtype=np.int64),
               cigar=((cols["end"].astype(np.int64) - cols["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(bam, ["chrA", "chrB"], dict(cols, **cig))
    try:
        fs = bamFragSizes(bam, GRanges(["chrA", "chrB"], [1, 1], width=REF_LEN, strand=["+", "*"]), tlenFilter=tf, verbose=False)
        assert np.array_equal(fs.counts, want)
        assert fs.mode() == length
        lo, hi = fs.tlen_filter(0.99)
        assert lo <= length <= hi and (lo, hi) != tf
        assert int(want[lo:hi + 1].sum()) * 100 >= 99 * fs.n
    finally:
        _lib.load().bsig_cache_clear()
