"""GPU: run-length coverage -- the encoder on raw device buffers (bsig_runs_*, csrc/runs.hip), on plans' results
(bsig_plan_runs_create) and through the file-level calls (bamCoverage / bamProfile with runs=True).  All exact.

The expected side is the plain numpy encoder of tests/runs_expected.py applied to the buffer itself (raw buffers), to
what the C oracle returns for the call (plans, blocks and slots), or to the goldens (the fixture BAM).  Never the
library's own per-range result: where that is looked at too, it is an extra assertion."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

import runs_expected as rx

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [2_000_000, 700_017]
CHUNK = 256
I32 = np.int32
MIN, MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---- the encoder on raw buffers ----------------------------------------------------------------------------------------
@pytest.fixture
def seams(monkeypatch):
    """a stretch is 256 cells: seams everywhere (read by bsig_runs_create)"""
    monkeypatch.setenv("BAMSIGNALS_RUNS_CHUNK_CELLS", str(CHUNK))


def _device(buf):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(buf, I32)).to("cuda:0") if len(buf) else torch.zeros(4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _encode(enc, buf):
    t = _device(buf)
    n = enc.encode(t.data_ptr())
    got = enc.fetch()
    assert n == enc.n_runs == len(got[1])
    del t
    return got


def _check_table(ctx, buf, base, length, stride=1):
    """encode `buf` by the table on the GPU; compare with the numpy encoder segment by segment"""
    from bamsignals_amd.device import RunEncoder
    enc = RunEncoder(ctx, base, length, stride)
    try:
        assert enc.n_seg == len(base) and enc.cells == int(np.sum(length))
        got = _encode(enc, buf)
    finally:
        enc.close()
    segs = rx.table_segments(buf, base, length, stride)
    rx.check_invariants(*got, segs)
    rx.same_runs(got, rx.encode_segments(segs))
    return got


def _cut(total, lens):
    """lengths that sum to total: the given ones, then the rest"""
    lens = list(lens) + [total - sum(lens)]
    return np.concatenate([[0], np.cumsum(lens)])[:-1], np.asarray(lens)


def test_all_cells_equal_is_one_run_per_segment(ctx, seams):
    n = 1 << 20
    base, length = _cut(n, [1, CHUNK - 1, CHUNK, CHUNK + 1, 100_000, 3 * CHUNK])
    seg_off, values, lengths = _check_table(ctx, np.full(n, 3, I32), base, length)
    assert seg_off.tolist() == list(range(8)) and lengths.tolist() == length.tolist()


def test_all_cells_different_is_one_run_per_cell(ctx, seams):
    n = 1 << 20
    base, length = _cut(n, [5, 70_000])
    seg_off, values, lengths = _check_table(ctx, np.arange(n, dtype=I32) - 1000, base, length)
    assert len(values) == n and np.all(lengths == 1)


def test_alternating_values(ctx, seams):
    n = (1 << 20) + 77
    base, length = _cut(n, [CHUNK * 10 + 1])
    _check_table(ctx, (np.arange(n) % 2).astype(I32), base, length)
    pairs = ((np.arange(n) // 2) % 2).astype(I32)               # 0 0 1 1: half as many runs
    got = _check_table(ctx, pairs, base, length)
    assert len(got[1]) < n // 2 + 3


@pytest.mark.parametrize("at", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + CHUNK // 2])
def test_one_change_at_and_off_a_seam(ctx, seams, at):
    n = 3 * CHUNK + 1
    buf = np.where(np.arange(n) < at, 5, 9).astype(I32)
    seg_off, values, lengths = _check_table(ctx, buf, [0], [n])
    assert values.tolist() == [5, 9] and lengths.tolist() == [at, n - at]


def test_segments_of_no_and_one_cell_and_no_segment(ctx, seams):
    buf = np.asarray([4, 4, 4, 2, 2, 8], I32)
    #            empty, one cell, empty, empty, three cells, empty x 2 at the end
    base, length = [0, 0, 1, 1, 3, 6, 6], [0, 1, 0, 0, 3, 0, 0]
    seg_off, values, lengths = _check_table(ctx, buf, base, length)
    assert seg_off.tolist() == [0, 0, 1, 1, 1, 3, 3, 3]
    assert values.tolist() == [4, 2, 8] and lengths.tolist() == [1, 2, 1]
    got = _check_table(ctx, buf, [2, 5], [0, 0])                # cells nowhere
    assert got[0].tolist() == [0, 0, 0] and len(got[1]) == 0
    got = _check_table(ctx, buf, [], [])                        # no segment
    assert got[0].tolist() == [0] and len(got[1]) == 0 and len(got[2]) == 0


def test_a_hundred_thousand_short_segments(ctx, seams):
    from bamsignals_amd.device import RunEncoder
    rng = np.random.default_rng(1)
    length = rng.integers(0, 6, 100_000)
    buf = rng.integers(0, 3, int(length.sum())).astype(I32)
    base = np.concatenate([[0], np.cumsum(length)])[:-1]
    enc = RunEncoder(ctx, base, length, 1)
    got = _encode(enc, buf)
    enc.close()
    rx.same_runs(got, rx.encode_many(buf, length))              # (the loop-free form of the same encoder: test_runs_cpu)
    rx.check_invariants(*got, rx.table_segments(buf, base, length, 1))
    assert len(buf) > len(got[1]) > 100_000 * 5 // 6


def test_equal_cells_on_both_sides_of_a_boundary_do_not_merge(ctx, seams):
    buf = np.asarray([1, 7, 7, 7, 7, 2], I32)
    seg_off, values, lengths = _check_table(ctx, buf, [0, 3], [3, 3])
    assert seg_off.tolist() == [0, 2, 4] and values.tolist() == [1, 7, 7, 2] and lengths.tolist() == [1, 2, 2, 1]
    # ... nor at a seam of stretches, nor where all cells are equal
    n = 4 * CHUNK
    seg_off, values, lengths = _check_table(ctx, np.full(n, 7, I32), [0, CHUNK, CHUNK + 1, 2 * CHUNK + 5], [CHUNK, 1, CHUNK + 4, 2 * CHUNK - 5])
    assert values.tolist() == [7] * 4 and lengths.tolist() == [CHUNK, 1, CHUNK + 4, 2 * CHUNK - 5]


def test_extreme_values_next_to_each_other(ctx, seams):
    cells = [MIN, MAX, -1, 0, 0, -1, -1, MAX, MAX, MIN, MIN, 0, MIN, -1, MAX]
    buf = np.tile(np.asarray(cells, I32), 40)
    seg_off, values, lengths = _check_table(ctx, buf, [0, 300], [300, 300])
    assert values[:7].tolist() == [MIN, MAX, -1, 0, -1, MAX, MIN] and lengths[:7].tolist() == [1, 1, 1, 2, 2, 2, 2]


def test_stride_two_rows_that_differ_and_rows_that_are_equal(ctx, seams):
    rng = np.random.default_rng(2)
    n = 10 * CHUNK + 3
    a, b = rng.integers(0, 2, n).astype(I32), rng.integers(0, 2, n).astype(I32) * 5
    for rows in ((a, b), (a, a)):
        buf = np.stack(rows, axis=1).reshape(-1)               # 2 * bin + row
        seg_off, values, lengths = _check_table(ctx, buf, [0, 1], [n, n], stride=2)
        for k in (0, 1):
            assert np.array_equal(np.repeat(values[seg_off[k]:seg_off[k + 1]], lengths[seg_off[k]:seg_off[k + 1]]), rows[k])
    # two ranges behind each other, as a strand-split plan lays them out
    buf = np.concatenate([np.stack((a, b), axis=1).reshape(-1), np.stack((b[:50], b[:50]), axis=1).reshape(-1)])
    _check_table(ctx, buf, [0, 1, 2 * n, 2 * n + 1], [n, n, 50, 50], stride=2)


def test_a_second_encode_gives_the_second_buffers_runs(ctx, seams):
    from bamsignals_amd.device import RunEncoder
    rng = np.random.default_rng(3)
    n = 5 * CHUNK
    base, length = _cut(n, [CHUNK + 7, 0, 1])
    enc = RunEncoder(ctx, base, length, 1)
    try:
        with pytest.raises(ValueError):
            enc.fetch()
        first = rng.integers(0, 2, n).astype(I32)
        second = np.full(n, 9, I32)                            # far fewer runs
        third = np.arange(n, dtype=I32)                        # far more
        for buf in (first, second, third, first):
            got = _encode(enc, buf)
            rx.same_runs(got, rx.encode_segments(rx.table_segments(buf, base, length, 1)))
        n_runs, so, va, le = enc.device_pointers()
        assert n_runs == len(got[1]) and so and va and le
    finally:
        enc.close()


def test_default_stretches(ctx):
    """without the knob: the stretch the library ships with"""
    rng = np.random.default_rng(4)
    n = 1_000_003
    buf = (rng.random(n) < 0.01).cumsum().astype(I32)           # long runs
    base, length = _cut(n, [2047, 2048, 2049, 300_000])
    _check_table(ctx, buf, base, length)


# ---- plans -------------------------------------------------------------------------------------------------------------
def _upload(ctx, cols):
    from bamsignals_amd.device import Reads
    if "cigar" in cols:
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                     cigar_off=cols["cigar_off"], cigar=cols["cigar"])
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])


@pytest.fixture(scope="module")
def synth(ctx):
    """paired reads on two references, resident on GPU 0, and the oracle's copy of them"""
    from bamsignals_amd.synth import synth_reads
    from oracle import oracle_c
    cols = synth_reads(400_000, REF_LEN, seed=92, paired=True)
    cols["end"] = oracle_c.cigar_end(cols["pos"], cols["flag"], cols["cigar_off"], cols["cigar"])
    reads = _upload(ctx, cols)
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    yield cols, reads, orc
    reads.close()


WIDTHS = (1, 100, 2048, 2049, 10_000)


def plan_ranges():
    """12 ranges of every width with mixed strands, then each whole reference; (ranges, group of every range)"""
    from bamsignals_amd.synth import synth_ranges
    parts = [synth_ranges(12, w, REF_LEN, seed=w) for w in WIDTHS]
    parts.append(dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[-1, 1]))
    rg = {k: np.concatenate([np.asarray(p[k], I32) for p in parts]) for k in ("rid", "loc", "len", "strand")}
    assert len(set(rg["strand"][:60].tolist())) == 3
    return rg, np.repeat(np.arange(len(parts)), [len(p["rid"]) for p in parts])


PE = dict(tlen_filter=(0, 1000), requiredF=66)
PLAN_CASES = (
    [("profile", dict(binsize=b, ss=ss, shift=sh)) for b in (1, 50) for ss in (False, True) for sh in (0, 75)]
    + [("profile", dict(binsize=1, ss=True, shift=0, pe_mid=True, **PE)), ("profile", dict(binsize=50, ss=False, shift=0, pe_mid=True, **PE))]
    + [("coverage", dict())]
    + [("coverage_ex", dict(binsize=b, ss=ss)) for b in (1, 7, 200) for ss in (False, True)]
    + [("coverage_ex", dict(binsize=7, ss=True, tspan=True, **PE)), ("coverage", dict(tspan=True, **PE))]
)
_cov_expected = {}


def expected_flat(kind, kw, cols, orc, rg):
    """(flat result, offsets, ss) of the call by the C oracle: bamProfile and per-base coverage straight from it, bins and
    strands of coverage as tests/test_coverage_binned_gpu.py derives them from its per-base coverage"""
    from oracle import oracle_c
    if kind == "profile":
        out, off = oracle_c.pileup_core(orc, rg, **kw)
        return out, off, kw["ss"]
    cov = {k: v for k, v in kw.items() if k not in ("binsize", "ss")}
    if kind == "coverage":
        out, off = oracle_c.coverage_core(orc, rg, **cov)
        return out, off, False
    from test_coverage_binned_gpu import Expected
    key = (id(cols), len(rg["len"]), int(np.sum(rg["len"])), tuple(sorted(cov.items())))
    if key not in _cov_expected:
        _cov_expected[key] = Expected(cols, rg, **cov)
    flat = _cov_expected[key].flat(kw["binsize"], kw["ss"])
    assert flat.max() <= MAX
    return flat.astype(I32), oracle_c.layout(rg["len"], kw["binsize"], kw["ss"]), kw["ss"]


def _mode(kind):
    from bamsignals_amd import _lib
    return dict(profile=_lib.MODE_PROFILE, coverage=_lib.MODE_COVERAGE, coverage_ex=_lib.MODE_COVERAGE_EX)[kind]


def plan_runs(ctx, reads, rg, kind, kw, times=2):
    """the plan's result encoded in HBM, `times` runs (the first with fused lookups, the later with the windows kept)
    which must agree; (runs, the per-range result as the plan wrote it, stats)"""
    import torch
    from bamsignals_amd.device import Plan, make_params
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_mode(kind), **kw))
    enc = plan.runs()
    try:
        assert enc.cells == plan.cells
        buf = torch.empty(max(plan.cells, 4), dtype=torch.int32, device="cuda:0")
        got = []
        for _ in range(times):
            buf.fill_(-7)
            torch.cuda.synchronize()
            plan.run_device(buf.data_ptr())
            ctx.sync()
            assert not plan.overflowed()
            enc.encode(buf.data_ptr())
            got.append(enc.fetch())
        for g in got[1:]:
            rx.same_runs(g, got[0])
        return got[0], buf.cpu().numpy()[:plan.cells], plan.stats()
    finally:
        enc.close()
        plan.close()


@pytest.mark.parametrize("kind,kw", PLAN_CASES, ids=[k + "-" + ",".join(f"{a}={b}" for a, b in kw.items() if a not in PE) for k, kw in PLAN_CASES])
def test_plans(ctx, synth, kind, kw):
    cols, reads, orc = synth
    rg, group = plan_ranges()
    flat, off, ss = expected_flat(kind, kw, cols, orc, rg)
    S = 2 if ss else 1
    segs = rx.flat_segments(flat, off, ss)
    want = rx.encode_segments(segs)
    got, cells, _ = plan_runs(ctx, reads, rg, kind, kw)
    assert len(got[0]) == len(rg["len"]) * S + 1
    rx.same_runs(got, want)
    rx.check_invariants(*got, segs)
    assert np.array_equal(cells, flat)                          # (extra: the per-range result the runs were made of)
    # not vacuous, on the expected side: the ranges of at least 100 bases together, and by width where a cell is a base
    seg_group = np.repeat(group, S)
    n_runs, n_cells = np.diff(want[0]), np.asarray([len(s) for s in segs])
    wide = seg_group >= 1
    assert wide.sum() < n_runs[wide].sum() < n_cells[wide].sum()
    if kw.get("binsize", 1) == 1:
        for g in range(1, len(WIDTHS) + 1):
            assert (seg_group == g).sum() < n_runs[seg_group == g].sum() < n_cells[seg_group == g].sum(), g


def test_heavy_tiles(ctx, monkeypatch):
    """a pile of reads on a few bases: their tiles are cut into slices that ADD after the main launch, so the encode must
    come after them"""
    from oracle import oracle_c
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    rng = np.random.default_rng(8)
    n = 6000
    pos = np.sort(np.concatenate([rng.integers(3000, 3005, n - 500), rng.integers(0, 49_000, 500)])).astype(I32)
    cols = dict(ref_len=np.asarray([50_000], I32), ref_off=np.asarray([0, n], np.int64), pos=pos, end=pos + rng.integers(30, 120, n).astype(I32),
                flag=np.where(rng.random(n) < 0.5, 16, 0).astype(np.uint16), mapq=np.full(n, 30, np.uint8), tlen=np.zeros(n, I32))
    reads = _upload(ctx, cols)
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    rg = dict(rid=np.zeros(4, I32), loc=np.asarray([0, 2900, 3002, 2000], I32), len=np.asarray([50_000, 300, 1, 2049], I32),
              strand=np.asarray([1, -1, 0, -1], I32))
    try:
        for kind, kw in (("profile", dict(binsize=1, ss=True, shift=0)), ("coverage", dict()), ("coverage_ex", dict(binsize=7, ss=True)),
                         ("profile", dict(binsize=50, ss=False, shift=10))):
            flat, off, ss = expected_flat(kind, kw, cols, orc, rg)
            got, cells, stats = plan_runs(ctx, reads, rg, kind, kw)
            assert stats["heavy_tiles"] > 0, (kind, kw)
            rx.same_runs(got, rx.encode_flat(flat, off, ss))
            assert flat.max() > 64
    finally:
        reads.close()


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors(ctx, synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, Plan, RunEncoder, SumPlan, XcorrPlan, make_params
    cols, reads, orc = synth
    a = ([0, 1], [100, 200], [500, 500], [1, -1])

    def refused(make):
        with pytest.raises(_lib.BsigError) as e:
            make()
        assert e.value.code_name == "BSIG_ERR_ARG"
    plans = [Plan(ctx, reads, *a, make_params(_lib.MODE_COUNT, binsize=-1)),
             SumPlan(ctx, reads, *a, make_params(_lib.MODE_PROFILE)),
             XcorrPlan(ctx, reads, *a, make_params(_lib.MODE_PROFILE, ss=True), 100),
             FragPlan(ctx, reads, *a, make_params(_lib.MODE_COUNT, binsize=-1, tlen_filter=(0, 1000), requiredF=66), 1)]
    import ctypes as C
    h = C.c_void_p()
    lib = _lib.load()
    try:
        for p in plans:
            refused(lambda: _lib.check(lib.bsig_plan_runs_create(p._h, C.byref(h))))
            assert not h.value
        refused(plans[0].runs)
    finally:
        for p in plans:
            p.close()
    refused(lambda: RunEncoder(ctx, [0, 10], [10, -1], 1))
    for stride in (0, 3, -1):
        refused(lambda: RunEncoder(ctx, [0], [10], stride))
    assert lib.bsig_runs_create(ctx._h, -1, None, None, 1, C.byref(h)) == -1 and not h.value
    enc = RunEncoder(ctx, [0], [10], 1)
    refused(enc.device_pointers)                                # nothing encoded yet
    enc.close()


# ---- file level: blocks and slots ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shuffled(fixture_reads):
    """60 ranges on the fixture BAM in no order: widths 1 .. 4,000, one wider than the block budget below, one empty"""
    from bamsignals_amd import GRanges
    fx = fixture_reads
    names = [str(s) for s in fx["ref_names"]]
    rng = np.random.default_rng(31)
    n = 60
    rid = rng.integers(0, len(names), n).astype(I32)
    w = rng.integers(1, 4000, n).astype(I32)
    w[17], w[40] = 7237, 0
    loc = np.asarray([rng.integers(0, int(fx["ref_len"][r]) - 100) for r in rid], I32)
    loc[17] = 3000
    strand = np.asarray([1, -1, 0], I32)[rng.integers(0, 3, n)]
    gr = GRanges([names[r] for r in rid], loc + 1, width=w, strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in strand])
    rg = dict(rid=rid, loc=loc, len=w, strand=strand)
    cols = dict(ref_off=fx["ref_off"], pos=fx["bam_pos"], end=fx["bam_end"], flag=fx["bam_flag"], mapq=fx["bam_mapq"], tlen=fx["bam_tlen"])
    return gr, rg, cols


def _blocks(route):
    m = re.search(r"runs of (\d+) block", route)
    assert m, route
    return int(m.group(1))


@pytest.mark.filterwarnings("ignore:some ranges' widths")
def test_blocks_and_slots(shuffled, monkeypatch):
    from bamsignals_amd import _lib, bamCoverage, bamProfile
    from bamsignals_amd.wrappers import last_call_route
    from oracle import oracle_c
    gr, rg, cols = shuffled
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    calls = (
        (lambda: bamCoverage(BAM, gr, runs=True, verbose=False), "coverage", dict()),
        (lambda: bamCoverage(BAM, gr, runs=True, binsize=7, ss=True, verbose=False), "coverage_ex", dict(binsize=7, ss=True)),
        (lambda: bamProfile(BAM, gr, runs=True, ss=True, shift=20, verbose=False), "profile", dict(binsize=1, ss=True, shift=20)),
    )
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        for call, kind, kw in calls:
            flat, off, ss = expected_flat(kind, kw, cols, orc, rg)
            want = rx.encode_flat(flat, off, ss)
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
            monkeypatch.delenv("BAMSIGNALS_RUNS_BLOCK_CELLS", raising=False)
            one = call()
            assert "1 GPU slot(s)" in last_call_route() and _blocks(last_call_route()) == 1
            rx.same_runs((one.seg_off, one.values, one.lengths), want)
            cells = np.diff(off)
            budget = int(cells.sum()) // 25                     # at least 25 blocks, and one range that is larger than a block
            assert cells.max() > budget
            monkeypatch.setenv("BAMSIGNALS_RUNS_BLOCK_CELLS", str(budget))
            many = call()
            assert "1 GPU slot(s)" in last_call_route() and _blocks(last_call_route()) >= 10
            rx.same_runs((many.seg_off, many.values, many.lengths), want)
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
            four = call()
            assert "4 GPU slot(s)" in last_call_route() and "runs" in last_call_route() and _blocks(last_call_route()) >= 10
            rx.same_runs((four.seg_off, four.values, four.lengths), want)
            monkeypatch.delenv("BAMSIGNALS_RUNS_BLOCK_CELLS", raising=False)
            four = call()
            assert "4 GPU slot(s)" in last_call_route() and _blocks(last_call_route()) == 4
            rx.same_runs((four.seg_off, four.values, four.lengths), want)
    finally:
        _lib.load().bsig_cache_clear()


# ---- file level: the fixture BAM against the goldens -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_gr(fixture_regions):
    from bamsignals_amd import GRanges
    reg, ranges = fixture_regions
    return GRanges(reg["chrom"], reg["start"], width=reg["width"], strand=reg["strand"]), ranges


def test_file_level_against_the_goldens(golden_gr, expected_grid, tmp_path, monkeypatch):
    from bamsignals_amd import RunSignals, _lib, bamCoverage, bamProfile
    from bamsignals_amd.wrappers import last_call_route, last_call_timing
    from oracle import oracle_c
    gr, ranges = golden_gr
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    monkeypatch.delenv("BAMSIGNALS_DEVICES", raising=False)
    _lib.load().bsig_cache_clear()
    try:
        # bamCoverage
        golden = expected_grid["coverage|mapq=0,pe=ignore,tf=NULL"]
        off = oracle_c.layout(ranges["len"], 1, False)
        want = rx.encode_flat(golden, off, False)
        sig = bamCoverage(BAM, gr, runs=True, verbose=False)
        assert isinstance(sig, RunSignals) and len(sig) == len(gr) and not sig.ss
        assert "runs" in last_call_route() and not last_call_timing()["bam_was_resident"]
        t = last_call_timing()
        assert t["plan"] > 0 and t["kernels"] > 0 and t["download"] > 0
        rx.same_runs((sig.seg_off, sig.values, sig.lengths), want)
        assert len(gr) < sig.nruns < len(golden)
        again = bamCoverage(BAM, gr, runs=True, verbose=False)               # resident
        assert last_call_timing()["bam_was_resident"] and "runs" in last_call_route()
        rx.same_runs((again.seg_off, again.values, again.lengths), want)
        plain = bamCoverage(BAM, gr, verbose=False)
        assert "runs" not in last_call_route()
        for i in range(len(gr)):
            assert np.array_equal(sig.decode(i), plain[i]) and np.array_equal(plain[i], golden[off[i]:off[i + 1]])
        # its bedGraph, range by range (ranges may overlap): read back and expanded it is the per-base coverage
        for i in (0, 1, 7, 20, 49):
            one = RunSignals(np.asarray([0, len(sig[i][0])]), sig[i][0], sig[i][1], False)
            path = tmp_path / f"r{i}.bedGraph"
            n_lines = one.to_bedgraph(path, gr[i:i + 1])
            base = golden[off[i]:off[i + 1]]
            ascending = base[::-1] if gr.strand[i] == "-" else base
            assert np.array_equal(rx.bedgraph_expand(path, gr.seqnames[i], gr.start[i], gr.width[i]), ascending)
            assert open(path).read().splitlines() == rx.bedgraph_lines([base], gr.seqnames[i:i + 1], gr.start[i:i + 1], gr.width[i:i + 1],
                                                                       gr.strand[i:i + 1]) and n_lines > 0
        path = tmp_path / "all.bedGraph"
        sig.to_bedgraph(path, gr)
        assert open(path).read().splitlines() == rx.bedgraph_lines([golden[off[i]:off[i + 1]] for i in range(len(gr))], gr.seqnames,
                                                                   gr.start, gr.width, gr.strand)
        # bamProfile, strand-specific
        golden = expected_grid["profile|shift=0,mapq=0,ss=1,pe=ignore,tf=NULL"]
        off = oracle_c.layout(ranges["len"], 1, True)
        sig = bamProfile(BAM, gr, runs=True, ss=True, verbose=False)
        assert sig.ss and len(sig) == len(gr) and "runs" in last_call_route()
        rx.same_runs((sig.seg_off, sig.values, sig.lengths), rx.encode_flat(golden, off, True))
        plain = bamProfile(BAM, gr, ss=True, verbose=False)
        for i in range(len(gr)):
            assert sig.decode(i).shape == plain[i].shape and np.array_equal(sig.decode(i), plain[i])
        # ... with a shift, midpoints and a filter: another golden
        golden = expected_grid["profile|shift=100,mapq=0,ss=1,pe=midpoint,tf=50_200"]
        sig = bamProfile(BAM, gr, runs=True, ss=True, shift=100, paired_end="midpoint", tlenFilter=(50, 200), verbose=False)
        rx.same_runs((sig.seg_off, sig.values, sig.lengths), rx.encode_flat(golden, off, True))
    finally:
        _lib.load().bsig_cache_clear()
