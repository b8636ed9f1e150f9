"""GPU: the strand cross-correlation over ranges (bsig_plan_create_xcorr, k_xcorr_tiles; bamCrossCorr) against the
oracle's per-range, per-base, strand-split pileup correlated in int64 (tests/crosscorr_expected.py).  All exact.

The overflow proof's refusal is not exercised: it needs the squared read counts of the tiles to add up to 2^63, i.e.
one tile with 3e9 reads in its windows or 4e8 tiles over a pile of 140,000 -- no input a test can hold."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import crosscorr_expected as xe
from test_crosscorr_cpu import LAG_MESSAGE, PARAM_RULE

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [2_000_000, 700_017]
CAP = 2047


def _upload(ctx, cols):
    from bamsignals_amd.device import Reads
    if "cigar" in cols:
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                     cigar_off=cols["cigar_off"], cigar=cols["cigar"])
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])


@pytest.fixture(scope="module")
def synth():
    """single-end and paired reads on two references, resident on GPU 0, and the oracle's copy of them"""
    from bamsignals_amd.device import Context
    from bamsignals_amd.synth import synth_reads
    from oracle import oracle_c
    ctx = Context(0)
    out = {}
    for paired in (False, True):
        cols = synth_reads(400_000, REF_LEN, seed=91 + paired, paired=paired)
        cols["end"] = oracle_c.cigar_end(cols["pos"], cols["flag"], cols["cigar_off"], cols["cigar"])
        out[paired] = (cols, _upload(ctx, cols), xe.oracle_reads(cols))
    yield ctx, out
    for _, r, _ in out.values():
        r.close()
    ctx.close()


def _params(**kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    return make_params(_lib.MODE_PROFILE, **kw)


def _run(ctx, reads, rg, maxlag, runs=2, **kw):
    """a plan's first run (fused lookups) and its later ones (windows kept), which must agree; (result, stats)"""
    from bamsignals_amd.device import XcorrPlan
    plan = XcorrPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(**kw), maxlag)
    try:
        assert plan.cells == maxlag + 6
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int64
        return got[0], plan.stats()
    finally:
        plan.close()


def _oracle_kw(kw):
    return {k: v for k, v in kw.items() if k in ("tlen_filter", "mapqual", "requiredF", "filteredF")}


def _check(ctx, reads, orc, rg, maxlag, runs=2, **kw):
    got, st = _run(ctx, reads, rg, maxlag, runs=runs, **kw)
    want = xe.flat(*xe.expected(orc, rg, maxlag, **_oracle_kw(kw)))
    assert np.array_equal(got, want), (maxlag, kw, np.flatnonzero(got != want)[:8])
    return got, st


def _ranges(n, w, seed, jitter=0):
    from bamsignals_amd.synth import synth_ranges
    return synth_ranges(n, w, REF_LEN, seed=seed, jitter=jitter)


def _cat(*rgs):
    return {k: np.concatenate([np.asarray(r[k], np.int32) for r in rgs]) for k in ("rid", "loc", "len", "strand")}


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 100, 1023, 1024, 1025, 2048, 2049, 10_000])
def test_grid(synth, w):
    ctx, data = synth
    rg = _ranges(60 if w < 10_000 else 12, w, seed=w)
    assert w >= 10_000 or len(set(rg["strand"].tolist())) == 3
    for paired in (False, True):
        cols, reads, orc = data[paired]
        for maxlag in (0, 1, 63, 64, 500):
            _check(ctx, reads, orc, rg, maxlag)
    _check(ctx, data[False][1], data[False][2], rg, CAP)


def test_whole_references_with_short_ranges(synth):
    """both references whole ('+' and '-'), short ranges, zero widths, duplicates, overhangs on both ends: one call"""
    ctx, data = synth
    whole = dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[1, -1])
    short = _ranges(40, 300, seed=8, jitter=290)
    edge = dict(rid=[0, 0, 1, 1, 0, 0, 1], loc=[-700, 1_999_500, -3, 700_000, 5000, 5000, 40], len=[1500, 900, 10, 600, 0, 777, 0],
                strand=[1, -1, 0, 1, 1, -1, 0])
    rg = _cat(whole, short, edge, short, dict(rid=[0, 0], loc=[5000, 5000], len=[777, 777], strand=[-1, -1]))
    cols, reads, orc = data[False]
    _check(ctx, reads, orc, rg, 500)
    _check(ctx, reads, orc, _cat(whole), CAP, runs=1)
    cols, reads, orc = data[True]
    _check(ctx, reads, orc, rg, 500, tlen_filter=(50, 500), requiredF=66)


def test_edges(synth):
    ctx, data = synth
    cols, reads, orc = data[False]
    got, st = _run(ctx, reads, dict(rid=[], loc=[], len=[], strand=[]), 500, runs=1)
    assert got.shape == (506,) and not got.any() and st["n_items"] == 0
    got, _ = _run(ctx, reads, dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1]), 7, runs=1)
    assert not got.any()
    # ranges narrower than maxlag
    _check(ctx, reads, orc, _ranges(50, 40, seed=4, jitter=39), 500)


def test_filters_threads_and_small_bodies(synth):
    ctx, data = synth
    rg = _ranges(40, 3000, seed=5, jitter=800)
    cols, reads, orc = data[False]
    for kw in (dict(mapqual=20), dict(filteredF=1024), dict(mapqual=30, filteredF=1024)):
        for threads in (64, 128, 256):
            _check(ctx, reads, orc, rg, 500, threads=threads, **kw)
    cols, reads, orc = data[True]
    for threads in (64, 256):
        _check(ctx, reads, orc, rg, 200, threads=threads, tlen_filter=(100, 300), requiredF=66)
    # bodies of 64 and 16 cells: a halo of 500 spans many bodies
    for body in (64, 16, 1000):
        got, st = _check(ctx, data[False][1], data[False][2], rg, 500, tile_cells=body)
        assert st["n_items"] == int(np.sum((rg["len"] + body - 1) // body))


@pytest.mark.parametrize("env", [{}, {"BAMSIGNALS_PACKED_HALF": "0"}, {"BAMSIGNALS_PACK": "0"}])
def test_packed_forms(synth, env, monkeypatch):
    ctx, data = synth
    cols, _, orc = data[False]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads = _upload(ctx, cols)
    try:
        got, st = _check(ctx, reads, orc, _ranges(80, 2500, seed=11), 300)
        if not env:
            assert st["bytes_per_visit_packed"] == 2          # the 16-bit column
    finally:
        reads.close()


def test_run_lengths(synth, monkeypatch):
    """one tile per workgroup, and all tiles in one"""
    ctx, data = synth
    cols, reads, orc = data[False]
    rg = _ranges(30, 5000, seed=13)
    for per in ("1", "1000000"):
        monkeypatch.setenv("BAMSIGNALS_XCORR_RUN_TILES", per)
        _check(ctx, reads, orc, rg, 100)


def test_wide_tiles_by_a_lowered_ceiling(synth, monkeypatch):
    ctx, data = synth
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    cols, reads, orc = data[False]
    got, st = _check(ctx, reads, orc, _ranges(40, 2049, seed=3), 500)
    assert st["heavy_tiles"] > 0


# ---- seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strand", [1, -1])
def test_seams(synth, strand):
    """forward 5' ends on the last and the first cell of a body, the partner 0, 1, maxlag - 1, maxlag, maxlag + 1 on"""
    ctx = synth[0]
    maxlag, body, loc, w = 100, 256, 1000, 256 * 3 + 130
    xs = [body - 1, body, 2 * body - 1, 2 * body, w - 1 - 50]            # (the last: its far partners cross the range's end)
    ds = [0, 1, maxlag - 1, maxlag, maxlag + 1]
    parts = []
    for x in xs:
        for d in ds:
            if strand > 0:      # the forward read is the sense one: its 5' end on cell x, its partner's d cells on
                f, r = loc + x, loc + x + d
                one = dict(rid=np.zeros(2, np.int64), pos=np.asarray([f, r - 29]), end=np.asarray([f + 29, r]), flag=np.asarray([0, 16]))
            else:               # mirrored, the REVERSE read is the sense one
                r, f = loc + w - 1 - x, loc + w - 1 - x - d
                one = dict(rid=np.zeros(2, np.int64), pos=np.asarray([r - 29, f]), end=np.asarray([r, f + 29]), flag=np.asarray([16, 0]))
            parts.append(one)
    cols = xe.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([50_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=[0], loc=[loc], len=[w], strand=[strand])
        want_c, want_m = xe.expected(cols, rg, maxlag)
        assert want_m[1] == len(xs) * len(ds) and want_c[maxlag] >= 4 and want_c[0] >= 5      # (the planting took)
        assert want_m[2] < want_m[1]                                      # ... and some partners lie beyond the range
        for b in (body, 64, 0):
            got, _ = _run(ctx, reads, rg, maxlag, tile_cells=b)
            assert np.array_equal(got, xe.flat(want_c, want_m)), b
    finally:
        reads.close()


# ---- piles -----------------------------------------------------------------------------------------------------------
def _pile(n_reads, d, at=50_000, beside=None):
    """n_reads forward reads with their 5' end on one base and as many reverse 5' ends d bases on"""
    f = dict(rid=np.zeros(n_reads, np.int64), pos=np.full(n_reads, at), end=np.full(n_reads, at + 39), flag=np.zeros(n_reads, np.int64))
    r = dict(rid=np.zeros(n_reads, np.int64), pos=np.full(n_reads, at + d - 39), end=np.full(n_reads, at + d), flag=np.full(n_reads, 16))
    cols = xe.merge_sorted([f, r] + ([beside] if beside else []), 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    return cols


@pytest.mark.parametrize("n_reads", [16_383, 16_384, 16_385, 32_766, 32_767, 32_768, 32_769, 70_000])
@pytest.mark.parametrize("beside", [False, True])
def test_piles_on_one_base(synth, n_reads, beside):
    """2 n reads in one tile's windows: the 32-bit image from 32,769 reads on; 70,000^2 = 4.9e9 is past 2^32"""
    ctx = synth[0]
    other = None
    if beside:
        rng = np.random.default_rng(n_reads)
        p = rng.integers(45_000, 56_000, 3000)
        other = dict(rid=np.zeros(3000, np.int64), pos=p, end=p + 49, flag=np.where(rng.random(3000) < 0.5, 16, 0))
    d = 150
    cols = _pile(n_reads, d, beside=other)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=np.zeros(4, np.int32), loc=np.asarray([49_000, 49_990, 48_000, 50_000 - 2047], np.int32),
                  len=np.asarray([3000, 3000, 2200, 2048 + 151], np.int32), strand=np.asarray([1, -1, 0, 1], np.int32))
        want = xe.flat(*xe.expected(cols, rg, 200))
        assert want[d] >= 3 * n_reads * n_reads
        got, st = _run(ctx, reads, rg, 200)
        assert np.array_equal(got, want)
        # the path taken: more than 32,768 reads in a tile's windows take the 32-bit image
        if 2 * n_reads > 32_768:
            assert st["heavy_tiles"] > 0
        elif 2 * n_reads + (3000 if beside else 0) <= 32_768:
            assert st["heavy_tiles"] == 0
        if n_reads == 70_000:
            assert got[d] > 2 ** 32 and st["heavy_tiles"] > 0
    finally:
        reads.close()


# ---- plans -----------------------------------------------------------------------------------------------------------
def test_stale_plan_and_wrong_run_calls(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, SumPlan, XcorrPlan
    ctx, data = synth
    cols, _, _ = data[False]
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        a = ([0], [10], [100], [1])
        xp = XcorrPlan(ctx, reads, *a, _params(), 20)
        pp, sp = Plan(ctx, reads, *a, _params(ss=True)), SumPlan(ctx, reads, *a, _params())
        b32, b64 = np.zeros(400, np.int32), np.zeros(400, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        for fn, plan, buf in ((lib.bsig_plan_run_host, xp, p32), (lib.bsig_plan_run_sum_host, xp, p64), (lib.bsig_plan_run, xp, p32),
                              (lib.bsig_plan_run_sum, xp, p64), (lib.bsig_plan_run_host_async, xp, p32),
                              (lib.bsig_plan_run_xcorr_host, pp, p64), (lib.bsig_plan_run_xcorr_host, sp, p64),
                              (lib.bsig_plan_run_xcorr, pp, p64), (lib.bsig_plan_run_xcorr, sp, p64)):
            assert fn(plan._h, buf) == -1
            assert "runs" in lib.bsig_last_error().decode()
        assert lib.bsig_plan_xcorr_cells(pp._h) == 0 and lib.bsig_plan_xcorr_cells(xp._h) == 26
        first = xp.run_host()
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        with pytest.raises(_lib.BsigError, match="make a new plan"):
            xp.run_host()
        xp2 = XcorrPlan(ctx, reads, *a, _params(), 20)
        assert np.array_equal(xp2.run_host(), first)
        for p in (xp, xp2, pp, sp):
            p.close()
    finally:
        reads.close()


def test_errors(synth):
    """the parameter rule's table (tests/test_crosscorr_cpu.py) and what only the plan call can express"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import XcorrPlan
    ctx, data = synth
    reads = data[False][1]
    a = ([0], [10], [100], [1])
    for kw, code, message in PARAM_RULE:
        kw = dict(kw)
        p = _lib.Params()
        p.mode, p.binsize, p.filteredF = _lib.MODE_PROFILE, 1, -1
        p.n_tlen_filter = len(kw.get("tlen_filter", ()))
        for i, v in enumerate(kw.get("tlen_filter", ())):
            p.tlen_filter[i] = v
        with pytest.raises(_lib.BsigError) as e:
            XcorrPlan(ctx, reads, *a, p, kw.get("max_lag", 10))
        assert (e.value.code, str(e.value)) == (code, message)
    for kw, message in ((dict(shift=1), "shift must be 0"), (dict(binsize=2), "binsize must be 1"),
                        (dict(pe_mid=True, tlen_filter=(0, 100)), "no paired-end midpoint rule"), (dict(threads=96), "threads must be")):
        with pytest.raises(_lib.BsigError, match=message) as e:
            XcorrPlan(ctx, reads, *a, _params(**kw), 10)
        assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError) as e:
        XcorrPlan(ctx, reads, *a, _lib.Params(mode=_lib.MODE_COUNT, binsize=1, filteredF=-1), 10)
    assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError, match=LAG_MESSAGE):
        XcorrPlan(ctx, reads, *a, _params(), CAP + 1)
    with pytest.raises(_lib.BsigError) as e:
        XcorrPlan(ctx, reads, [5], [10], [100], [1], _params(), 10)
    assert e.value.code_name == "BSIG_ERR_CHROM"


# ---- file level ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(fixture_reads):
    from bamsignals_amd import GRanges
    fx = fixture_reads
    names = [str(s) for s in fx["ref_names"]]
    rng = np.random.default_rng(23)
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


def test_file_level(fixture, decode_mode):
    from bamsignals_amd import bamCrossCorr
    from bamsignals_amd.wrappers import flagMask, tlenFilter
    gr, rg, cols = fixture
    for pe, tf, kw in (("ignore", None, dict()), ("filter", None, dict(mapqual=10)), ("filter", (50, 300), dict(filteredFlag=1024))):
        for maxlag in (500, 0, CAP):
            cc = bamCrossCorr(BAM, gr, maxlag=maxlag, paired_end=pe, tlenFilter=tf, verbose=False, **kw)
            cross, mom = xe.expected(cols, rg, maxlag, tlen_filter=tlenFilter(tf, pe), requiredF=flagMask(pe),
                                     mapqual=kw.get("mapqual", 0), filteredF=kw.get("filteredFlag", -1))
            assert np.array_equal(cc.cross, cross) and cc.cross.dtype == np.int64, (pe, maxlag)
            assert [cc.n_cells, *cc.sums, *cc.sumsqs] == mom.tolist()
    assert mom[1] > 0


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import bamCrossCorr
    from bamsignals_amd.wrappers import last_call_route
    from bamsignals_amd import _lib
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
        one = bamCrossCorr(BAM, gr, maxlag=300, verbose=False)
        assert "1 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
        four = bamCrossCorr(BAM, gr, maxlag=300, verbose=False)
        assert "4 GPU slot(s)" in last_call_route() and "sum" in last_call_route()
        assert np.array_equal(one.cross, four.cross) and one.cross.any()
        assert (one.n_cells, one.sums, one.sumsqs) == (four.n_cells, four.sums, four.sumsqs)
    finally:
        _lib.load().bsig_cache_clear()


# ---- the use ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [147, 200, 431])
def test_fragment_length_is_read_off_the_data(synth, length, tmp_path):
    """20,000 fragments of one length over 400,000 background reads: fragment_length() is that length"""
    from bamsignals_amd import CrossCorr, GRanges, bamCrossCorr, write_columns_as_bam
    from bamsignals_amd import _lib
    ctx, data = synth
    bg = data[False][0]
    ref_off = np.asarray(bg["ref_off"])
    parts = [dict(rid=np.repeat(np.arange(2), np.diff(ref_off)), pos=bg["pos"], end=bg["end"], flag=bg["flag"], mapq=bg["mapq"]),
             xe.fragments(20_000, length, REF_LEN[0], seed=length)]
    cols = xe.merge_sorted(parts, 2)
    cols["ref_len"] = np.asarray(REF_LEN, np.int64)
    rg = dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[1, 0])
    cross, mom = xe.expected(cols, rg, 500)
    assert int(np.argmax(cross)) == length - 1 and np.sum(cross == cross.max()) == 1      # the oracle's own maximum, unique
    reads = _upload(ctx, cols)
    try:
        got, _ = _run(ctx, reads, rg, 500)
    finally:
        reads.close()
    assert np.array_equal(got, xe.flat(cross, mom))
    cc = CrossCorr(got[:501], got[501], got[502:504], got[504:506])
    assert cc.fragment_length() == length
    r = cc.correlation()
    assert int(np.argmax(r)) == length - 1 and 0 < r[length - 1] < 1
    # ... and through a BAM file and the user's call
    bam = str(tmp_path / "frag.bam")
    cig = dict(cigar_off=np.arange(len(cols["pos"]) + 1, dtype=np.int64),
               cigar=((cols["end"].astype(np.int64) - cols["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(bam, ["chrA", "chrB"], dict(cols, **cig))
    try:
        cc2 = bamCrossCorr(bam, GRanges(["chrA", "chrB"], [1, 1], width=REF_LEN, strand=["+", "*"]), verbose=False)
        assert np.array_equal(cc2.cross, cross) and cc2.fragment_length() == length
    finally:
        _lib.load().bsig_cache_clear()
