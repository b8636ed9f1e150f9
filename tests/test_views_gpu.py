"""GPU: bamViews -- the views encoder on raw device buffers (bsig_views_*, csrc/views.hip), on plans' results
(bsig_plan_views_create) and through the file-level calls (bamViews).  All exact.

The expected side is the plain numpy of tests/views_expected.py applied to the buffer itself (raw buffers), to what the
C oracle returns for the call (plans, blocks and slots), or to the goldens (the fixture BAM).  Never the library's own
views, never its per-range result: where that is looked at too, it is an extra assertion."""
import os
import re
import warnings

import numpy as np
import pytest

from conftest import GOLDEN

import resized_expected
import views_expected as vx

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
    """a stretch is 256 cells: seams everywhere (read by bsig_views_create)"""
    monkeypatch.setenv("BAMSIGNALS_VIEWS_CHUNK_CELLS", str(CHUNK))


def _device(buf):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(buf, I32)).to("cuda:0") if len(buf) else torch.zeros(4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _encode(enc, buf, lower, upper=MAX):
    t = _device(buf)
    n = enc.encode(t.data_ptr(), lower, upper)
    got = enc.fetch()
    assert n == enc.n_views == len(got[1])
    del t
    return got


def _check_table(ctx, buf, base, length, lower, upper=MAX, stride=1):
    """the views of `buf` by the table on the GPU; compared with numpy segment by segment"""
    from bamsignals_amd.device import ViewEncoder
    enc = ViewEncoder(ctx, base, length, stride)
    try:
        assert enc.n_seg == len(base) and enc.cells == int(np.sum(length))
        got = _encode(enc, buf, lower, upper)
    finally:
        enc.close()
    segs = vx.table_segments(buf, base, length, stride)
    vx.check_invariants(got, segs, lower, upper)
    vx.same_views(got, vx.views_of_segments(segs, lower, upper))
    return got


def _cut(total, lens):
    """lengths that sum to total: the given ones, then the rest"""
    lens = list(lens) + [total - sum(lens)]
    return np.concatenate([[0], np.cumsum(lens)])[:-1], np.asarray(lens)


def test_no_view_at_all(ctx, seams):
    n = 10 * CHUNK + 3
    base, length = _cut(n, [CHUNK, 0, 1])
    got = _check_table(ctx, np.full(n, 4, I32), base, length, 5)
    assert got[0].tolist() == [0] * 5 and all(len(a) == 0 for a in got[1:])
    from bamsignals_amd.device import ViewEncoder
    enc = ViewEncoder(ctx, base, length, 1)
    t = _device(np.full(n, 4, I32))
    assert enc.encode(t.data_ptr(), 5) == 0
    assert enc.device_pointers()[0] == 0 and enc.device_pointers()[1] and not any(enc.device_pointers()[2:])
    enc.close()


def test_one_view_over_a_million_cells_and_the_same_cut_into_segments(ctx, seams):
    n = 1 << 20
    buf = np.full(n, 5000, I32)
    seg_off, start, width, total, vmax, summit = _check_table(ctx, buf, [0], [n], 20)
    assert (start.tolist(), width.tolist(), total.tolist(), vmax.tolist(), summit.tolist()) == ([0], [n], [5000 * n], [5000], [0])
    assert total[0] > 2**32                                     # 4,096 stretches added into one slot
    # equal in-cells on both sides of a boundary do not merge, at a seam and off it
    base, length = _cut(n, [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 100])
    seg_off, start, width, total, vmax, summit = _check_table(ctx, buf, base, length, 20)
    assert len(length) == 6 and seg_off.tolist() == list(range(7)) and width.tolist() == length.tolist()
    assert not start.any() and not summit.any() and total.tolist() == (5000 * length).tolist()


@pytest.mark.parametrize("at", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + CHUNK // 2])
def test_a_view_that_ends_and_one_that_begins_at_and_off_a_seam(ctx, seams, at):
    n = 3 * CHUNK + 1
    ramp = (np.arange(n) % 37 + 3).astype(I32)
    ends = np.where(np.arange(n) <= at, ramp, 0).astype(I32)    # its last cell is `at`
    got = _check_table(ctx, ends, [0], [n], 1)
    assert got[1].tolist() == [0] and got[2].tolist() == [at + 1]
    begins = np.where(np.arange(n) >= at, ramp, 0).astype(I32)
    got = _check_table(ctx, begins, [0], [n], 1)
    assert got[1].tolist() == [at] and got[2].tolist() == [n - at]
    both = np.where(np.arange(n) == at, 0, ramp).astype(I32)    # one ends in front of `at`, one begins behind it
    got = _check_table(ctx, both, [0], [n], 1)
    assert got[1].tolist() == [0, at + 1] and got[2].tolist() == [at, n - at - 1]


def test_alternating_in_and_out(ctx, seams):
    n = (1 << 20) + 77
    base, length = _cut(n, [CHUNK * 10 + 1])
    got = _check_table(ctx, (np.arange(n) % 2 * 3).astype(I32), base, length, 1)
    assert len(got[1]) == n // 2 and np.all(got[2] == 1)
    pairs = ((np.arange(n) // 2) % 2 * (np.arange(n) % 5 + 1)).astype(I32)      # 0 0 x y: half as many views, two cells each
    got = _check_table(ctx, pairs, base, length, 1)
    assert n // 4 - 2 <= len(got[1]) <= n // 4 + 2 and got[2].max() == 2


def test_ties_of_the_max(ctx, seams):
    n = 4 * CHUNK
    flat = np.full(n, 3, I32)
    a = flat.copy()
    a[[10, 700]] = 9                                            # the same max in the first and in the third stretch
    assert _check_table(ctx, a, [0], [n], 1)[5].tolist() == [10]
    b = flat.copy()
    b[[2 * CHUNK + 5, 2 * CHUNK + 6]] = 9                       # the max only in the third stretch
    assert _check_table(ctx, b, [0], [n], 1)[5].tolist() == [2 * CHUNK + 5]
    down = np.arange(n, 0, -1).astype(I32)
    got = _check_table(ctx, down, [0], [n], 1)
    assert got[4].tolist() == [n] and got[5].tolist() == [0]
    up = np.arange(1, n + 1).astype(I32)
    got = _check_table(ctx, up, [0], [n], 1)
    assert got[4].tolist() == [n] and got[5].tolist() == [n - 1]
    # all equal, in several views: the first cell of each
    c = flat.copy()
    c[[100, CHUNK, 3 * CHUNK - 1]] = 0
    assert _check_table(ctx, c, [0], [n], 3, 3)[5].tolist() == [0, 101, CHUNK + 1, 3 * CHUNK]


def test_signed_values(ctx, seams):
    cells = [MIN, MAX, -1, 0, 0, -1, -1, MAX, MAX, MIN, MIN, 0, MIN, -1, MAX]
    buf = np.tile(np.asarray(cells, I32), 40)
    for lower, upper in ((MIN, -1), (0, 0), (MIN, MAX), (MAX, MAX)):
        got = _check_table(ctx, buf, [0, 300], [300, 300], lower, upper)
        assert len(got[1]) > 0
    got = _check_table(ctx, buf, [0, 300], [300, 300], MIN, MAX)
    assert got[0].tolist() == [0, 1, 2] and got[2].tolist() == [300, 300] and got[4].tolist() == [MAX, MAX] and got[5].tolist() == [1, 1]
    # three neighbours of INT32_MAX: the sum needs 64 bits; and of INT32_MIN
    buf = np.zeros(3 * CHUNK, I32)
    buf[CHUNK - 1:CHUNK + 2] = MAX
    buf[500:503] = MIN
    got = _check_table(ctx, buf, [0], [3 * CHUNK], 1)
    assert got[3].tolist() == [3 * MAX] and got[5].tolist() == [CHUNK - 1]
    got = _check_table(ctx, buf, [0], [3 * CHUNK], MIN, -1)
    assert got[3].tolist() == [3 * MIN] and got[4].tolist() == [MIN] and got[5].tolist() == [500]


def test_a_band(ctx, seams):
    rng = np.random.default_rng(11)
    n = 9 * CHUNK + 5
    buf = rng.integers(0, 6, n).astype(I32)
    buf[CHUNK - 4:CHUNK + 4] = [0, 2, 3, 2, 3, 5, 2, 1]         # a cell above the band breaks a view as one below it does
    got = _check_table(ctx, buf, [0], [n], 2, 3)
    k = int(np.searchsorted(got[1], CHUNK - 3))
    assert got[1][k:k + 2].tolist() == [CHUNK - 3, CHUNK + 2] and got[2][k] == 4
    assert got[4].max() == 3 and got[4].min() >= 2


def test_segments_of_no_and_one_cell_and_no_segment(ctx, seams):
    buf = np.asarray([4, 4, 4, 2, 2, 8], I32)
    #            empty, one cell, empty, empty, three cells, empty x 2 at the end
    base, length = [0, 0, 1, 1, 3, 6, 6], [0, 1, 0, 0, 3, 0, 0]
    got = _check_table(ctx, buf, base, length, 3)
    assert got[0].tolist() == [0, 0, 1, 1, 1, 2, 2, 2]
    assert got[1].tolist() == [0, 2] and got[2].tolist() == [1, 1] and got[3].tolist() == [4, 8] and got[5].tolist() == [0, 2]
    got = _check_table(ctx, buf, base, length, 9)               # ... and none of them in
    assert got[0].tolist() == [0] * 8
    got = _check_table(ctx, buf, [2, 5], [0, 0], 1)             # cells nowhere
    assert got[0].tolist() == [0, 0, 0] and len(got[1]) == 0
    got = _check_table(ctx, buf, [], [], 1)                     # no segment
    assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:])


def test_one_cell_segments_all_in_are_as_many_views_as_cells(ctx, seams):
    """a segment boundary ends a view, so in-cells on both sides of it are two views with no cell between them"""
    rng = np.random.default_rng(12)
    n = 3 * CHUNK + 7
    buf = rng.integers(1, 9, n).astype(I32)
    got = _check_table(ctx, buf, np.arange(n), np.ones(n, I32), 1)
    assert got[0].tolist() == list(range(n + 1)) and np.array_equal(got[3], buf) and not got[1].any() and np.all(got[2] == 1)
    got = _check_table(ctx, buf[:3], [0, 1, 2], [1, 1, 1], 1)   # three views over three cells
    assert got[0].tolist() == [0, 1, 2, 3]
    # one and two cells, empty segments between them, nearly all in
    length = rng.integers(0, 3, 700)
    buf = (rng.integers(1, 9, int(length.sum())) * (rng.random(int(length.sum())) < 0.95)).astype(I32)
    got = _check_table(ctx, buf, np.concatenate([[0], np.cumsum(length)])[:-1], length, 1)
    assert len(got[1]) > len(buf) // 2 + 1
    # one bin per row of a strand-split plan: 2 * range + antisense, stride 2
    m = 2 * CHUNK + 3
    buf = rng.integers(1, 9, 2 * m).astype(I32)
    got = _check_table(ctx, buf, np.arange(2 * m), np.ones(2 * m, I32), 1, stride=2)
    assert len(got[1]) == 2 * m and np.array_equal(got[3], buf)


@pytest.mark.parametrize("chunk", [100, 333])
def test_a_stretch_that_is_no_multiple_of_64(ctx, monkeypatch, chunk):
    """the last round of every stretch is partial, with more stretches behind it"""
    monkeypatch.setenv("BAMSIGNALS_VIEWS_CHUNK_CELLS", str(chunk))
    rng = np.random.default_rng(13)
    n = 41 * chunk + 17
    _check_table(ctx, np.full(n, 7, I32), [0], [n], 1)                              # one view over every seam
    base, length = _cut(n, [1, chunk - 1, chunk, chunk + 1, 0, 5 * chunk + 63])
    _check_table(ctx, np.full(n, 7, I32), base, length, 1)
    ramp = (np.arange(n) % 37 + 3).astype(I32)
    for at in (63, 64, chunk - 1, chunk, chunk + 1, chunk + 63, chunk + 64, 2 * chunk - 1, 2 * chunk):
        got = _check_table(ctx, np.where(np.arange(n) == at, 0, ramp).astype(I32), [0], [n], 1)
        assert got[1].tolist() == [0, at + 1] and got[2].tolist() == [at, n - at - 1]
    for dens in (0.05, 0.5, 0.95):
        buf = (rng.integers(1, 9, n) * (rng.random(n) < dens)).astype(I32)
        _check_table(ctx, buf, base, length, 1)
        _check_table(ctx, buf, base, length, 3, 6)
    _check_table(ctx, (np.arange(n) % 2).astype(I32), base, length, 1)
    rows = np.stack((ramp, rng.integers(0, 3, n).astype(I32)), axis=1).reshape(-1)
    _check_table(ctx, rows, [0, 1], [n, n], 1, stride=2)


def test_a_hundred_thousand_short_segments(ctx, seams):
    from bamsignals_amd.device import ViewEncoder
    rng = np.random.default_rng(1)
    length = rng.integers(0, 6, 100_000)
    buf = rng.integers(0, 3, int(length.sum())).astype(I32)
    base = np.concatenate([[0], np.cumsum(length)])[:-1]
    enc = ViewEncoder(ctx, base, length, 1)
    got = _encode(enc, buf, 1)
    enc.close()
    want = vx.views_of_many(buf, length, 1)                     # (the loop-free form of the same numpy: test_views_cpu)
    # five segments in six hold a cell, and two cells in three are in: more than 5/6 * 2/3 of the segments hold a view
    assert 55_000 < len(want[1]) < len(buf) and np.any(np.diff(want[0])[length > 0] == 0) and want[2].max() > 1
    vx.same_views(got, want)
    some = slice(40_000, 42_000)                                # ... and the invariants on two thousand of them
    a, b = int(got[0][some.start]), int(got[0][some.stop])
    part = (got[0][some.start:some.stop + 1] - a,) + tuple(x[a:b] for x in got[1:])
    vx.check_invariants(part, vx.table_segments(buf, base[some], length[some], 1), 1)


def test_stride_two_rows_that_differ_and_rows_that_are_equal(ctx, seams):
    rng = np.random.default_rng(2)
    n = 10 * CHUNK + 3
    a, b = rng.integers(0, 4, n).astype(I32), (rng.integers(0, 2, n) * rng.integers(1, 9, n)).astype(I32)
    for rows in ((a, b), (a, a)):
        buf = np.stack(rows, axis=1).reshape(-1)               # 2 * bin + row
        got = _check_table(ctx, buf, [0, 1], [n, n], 2, stride=2)
        for k in (0, 1):
            vx.same_views(tuple(x[got[0][k]:got[0][k + 1]] for x in got[1:]), vx.views_of(rows[k], 2))
    # two ranges behind each other, as a strand-split plan lays them out
    buf = np.concatenate([np.stack((a, b), axis=1).reshape(-1), np.stack((b[:50], b[:50]), axis=1).reshape(-1)])
    _check_table(ctx, buf, [0, 1, 2 * n, 2 * n + 1], [n, n, 50, 50], 2, stride=2)


def test_several_encodes_on_one_object(ctx, seams):
    from bamsignals_amd.device import ViewEncoder
    rng = np.random.default_rng(3)
    n = 5 * CHUNK
    base, length = _cut(n, [CHUNK + 7, 0, 1])
    enc = ViewEncoder(ctx, base, length, 1)
    try:
        with pytest.raises(ValueError):
            enc.fetch()
        few = np.where(np.arange(n) % 400 < 300, 9, 0).astype(I32)
        many = rng.integers(0, 2, n).astype(I32) * 9
        counts = []
        for buf, lower, upper in ((few, 1, MAX), (many, 9, 9), (many, 10, MAX), (many, 0, 0), (few, 9, MAX)):
            got = _encode(enc, buf, lower, upper)
            vx.same_views(got, vx.views_of_segments(vx.table_segments(buf, base, length, 1), lower, upper))
            counts.append(len(got[1]))
        assert counts[0] < 30 < counts[1] and counts[2] == 0 and counts[3] > 30 and counts[4] == counts[0]
        ptrs = enc.device_pointers()
        assert ptrs[0] == counts[4] and all(ptrs[1:])
    finally:
        enc.close()


def test_default_stretches(ctx, monkeypatch):
    """without the knob: the stretch the library ships with"""
    monkeypatch.delenv("BAMSIGNALS_VIEWS_CHUNK_CELLS", raising=False)
    rng = np.random.default_rng(4)
    n = 1_000_003
    buf = (20 + np.cumsum(rng.integers(-1, 2, n) * (rng.random(n) < 0.05))).astype(I32)      # slowly varying
    base, length = _cut(n, [2047, 2048, 2049, 300_000])
    lower = int(np.median(buf)) + 1
    got = _check_table(ctx, buf, base, length, lower)
    assert len(got[1]) > 5 and got[2].max() > 4096              # a view across several default stretches


# ---- plans -------------------------------------------------------------------------------------------------------------
def _upload(ctx, cols):
    from bamsignals_amd.device import Reads
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
    """12 ranges of every width with mixed strands, then each whole reference (the ranges of tests/test_runs_gpu.py)"""
    from bamsignals_amd.synth import synth_ranges
    parts = [synth_ranges(12, w, REF_LEN, seed=w) for w in WIDTHS]
    parts.append(dict(rid=[0, 1], loc=[0, 0], len=REF_LEN, strand=[-1, 1]))
    rg = {k: np.concatenate([np.asarray(p[k], I32) for p in parts]) for k in ("rid", "loc", "len", "strand")}
    assert len(set(rg["strand"][:60].tolist())) == 3
    return rg


PE = dict(tlen_filter=(0, 1000), requiredF=66)
PLAN_CASES = (
    [("profile", dict(binsize=b, ss=ss, shift=sh), 0) for b in (1, 50) for ss in (False, True) for sh in (0, 75)]
    + [("coverage", dict(), 0), ("coverage_ex", dict(binsize=7, ss=True), 0), ("coverage", dict(tspan=True, **PE), 0),
       ("coverage", dict(), 180)]
)
_expected = {}


def expected_flat(kind, kw, frag_len, cols, orc, rg):
    """(flat result, offsets, ss) of the call by the C oracle (kept per case: the reference is computed once)"""
    from oracle import oracle_c
    key = (id(cols), len(rg["len"]), kind, frag_len, tuple(sorted(kw.items())))
    if key not in _expected:
        if kind == "profile":
            out, off = oracle_c.pileup_core(orc, rg, **kw)
            ss = kw["ss"]
        else:
            flt = {k: v for k, v in kw.items() if k not in ("binsize", "ss")}
            b, ss = kw.get("binsize", 1), kw.get("ss", False)
            if frag_len:
                out, off = resized_expected.expected(cols, rg, frag_len, b, ss, **flt)
            elif kind == "coverage":
                out, off = oracle_c.coverage_core(orc, rg, **flt)
            else:
                out, off = resized_expected.coverage(cols, rg, b, ss, **flt)
                assert out.max() <= MAX
        out = np.asarray(out).astype(I32)
        out.setflags(write=False)
        _expected[key] = (out, off, ss)
    return _expected[key]


def lower_of(flat):
    """the smallest value >= 1 that at most one cell in ten reaches: from the expected side"""
    counts = np.bincount(np.minimum(flat[flat >= 0], 1 << 16).astype(np.int64))
    reach = np.cumsum(counts[::-1])[::-1]                       # cells >= v
    return max(1, int(np.argmax(reach <= len(flat) // 10)))


def _mode(kind):
    from bamsignals_amd import _lib
    return dict(profile=_lib.MODE_PROFILE, coverage=_lib.MODE_COVERAGE, coverage_ex=_lib.MODE_COVERAGE_EX)[kind]


def plan_views(ctx, reads, rg, kind, kw, frag_len, lower, upper=MAX, times=2):
    """the views of the plan's result in HBM, `times` runs (the first with fused lookups, the later with the windows kept)
    which must agree; (views, the per-range result as the plan wrote it, stats)"""
    import torch
    from bamsignals_amd.device import Plan, make_params
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_mode(kind), **kw), frag_len=frag_len)
    enc = plan.views()
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
            enc.encode(buf.data_ptr(), lower, upper)            # (after the sync: heavy tiles' slices have been added)
            got.append(enc.fetch())
        for g in got[1:]:
            vx.same_views(g, got[0])
        return got[0], buf.cpu().numpy()[:plan.cells], plan.stats()
    finally:
        enc.close()
        plan.close()


@pytest.mark.parametrize("kind,kw,frag_len", PLAN_CASES,
                         ids=[k + "-" + ",".join(f"{a}={b}" for a, b in kw.items() if a not in PE) + (f",frag_len={f}" if f else "") for k, kw, f in PLAN_CASES])
def test_plans(ctx, synth, kind, kw, frag_len):
    cols, reads, orc = synth
    rg = plan_ranges()
    flat, off, ss = expected_flat(kind, kw, frag_len, cols, orc, rg)
    S = 2 if ss else 1
    segs = vx.flat_segments(flat, off, ss)
    lower = lower_of(flat)
    assert lower >= 1 and (flat >= lower).sum() * 10 <= len(flat) and (lower == 1 or (flat >= lower - 1).sum() * 10 > len(flat))
    want = vx.views_of_segments(segs, lower)
    # not vacuous, on the expected side alone
    assert len(want[1]) > len(rg["len"]) and want[2].max() > 1 and np.any(np.diff(want[0])[[len(s) > 0 for s in segs]] == 0)
    got, cells, _ = plan_views(ctx, reads, rg, kind, kw, frag_len, lower)
    assert len(got[0]) == len(rg["len"]) * S + 1
    vx.same_views(got, want)
    assert np.array_equal(cells, flat)                          # (extra: the per-range result the views were made of)
    small = [k for k, s in enumerate(segs) if len(s) <= 10_000]
    a = np.concatenate([np.arange(got[0][k], got[0][k + 1]) for k in small]).astype(np.int64)
    part = (np.concatenate([[0], np.cumsum([got[0][k + 1] - got[0][k] for k in small])]).astype(np.int64),) + tuple(x[a] for x in got[1:])
    vx.check_invariants(part, [segs[k] for k in small], lower)


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
            flat, off, ss = expected_flat(kind, kw, 0, cols, orc, rg)
            got, cells, stats = plan_views(ctx, reads, rg, kind, kw, 0, 65)
            assert stats["heavy_tiles"] > 0, (kind, kw)
            want = vx.views_of_segments(vx.flat_segments(flat, off, ss), 65)
            vx.same_views(got, want)
            assert flat.max() > 64 and want[4].max() == flat.max() and len(want[1]) > 0
    finally:
        reads.close()


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors(ctx, synth):
    import ctypes as C
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, Plan, SumPlan, ViewEncoder, XcorrPlan, make_params
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
    h = C.c_void_p()
    lib = _lib.load()
    try:
        for p in plans:
            refused(lambda: _lib.check(lib.bsig_plan_views_create(p._h, C.byref(h))))
            assert not h.value
        refused(plans[0].views)
    finally:
        for p in plans:
            p.close()
    refused(lambda: ViewEncoder(ctx, [0, 10], [10, -1], 1))
    for stride in (0, 3):
        refused(lambda: ViewEncoder(ctx, [0], [10], stride))
    assert lib.bsig_views_create(ctx._h, -1, None, None, 1, C.byref(h)) == -1 and not h.value
    enc = ViewEncoder(ctx, [0], [10], 1)
    refused(enc.device_pointers)                                # nothing encoded yet
    t = _device(np.arange(10))
    refused(lambda: enc.encode(t.data_ptr(), 3, 2))             # lower above upper
    with pytest.raises(ValueError):
        enc.fetch()                                             # ... and the refused encode left no result
    assert enc.encode(t.data_ptr(), 3, 3) == 1
    enc.close()


# ---- file level: blocks and slots ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shuffled(fixture_reads):
    """60 ranges on the fixture BAM in no order: widths 1 .. 4,000, one wider than the block budget below, one empty (the
    ranges of tests/test_runs_gpu.py)"""
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
    m = re.search(r"result: views of (\d+) block\(s\) of ranges, put in order on the host", route)
    assert m, route
    return int(m.group(1))


def _fields(sv):
    return tuple(getattr(sv, f) for f in vx.NAMES)


@pytest.mark.filterwarnings("ignore:some ranges' widths")
def test_blocks_and_slots(shuffled, monkeypatch):
    from bamsignals_amd import SignalViews, _lib, bamViews
    from bamsignals_amd.wrappers import last_call_route
    from oracle import oracle_c
    gr, rg, cols = shuffled
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    calls = (
        (lambda lo: bamViews(BAM, gr, lo, verbose=False), "coverage", dict()),
        (lambda lo: bamViews(BAM, gr, lo, binsize=7, ss=True, verbose=False), "coverage_ex", dict(binsize=7, ss=True)),
        (lambda lo: bamViews(BAM, gr, lo, signal="ends", ss=True, shift=20, verbose=False), "profile", dict(binsize=1, ss=True, shift=20)),
    )
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        for call, kind, kw in calls:
            flat, off, ss = expected_flat(kind, kw, 0, cols, orc, rg)
            lower = lower_of(flat)
            want = vx.views_of_segments(vx.flat_segments(flat, off, ss), lower)
            assert len(want[1]) > len(gr)
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
            monkeypatch.delenv("BAMSIGNALS_RUNS_BLOCK_CELLS", raising=False)
            one = call(lower)
            assert isinstance(one, SignalViews) and one.ss == ss and len(one) == len(gr)
            assert "1 GPU slot(s)" in last_call_route() and _blocks(last_call_route()) == 1
            vx.same_views(_fields(one), want)
            cells = np.diff(off)
            budget = int(cells.sum()) // 25                     # at least 25 blocks, and one range that is larger than a block
            assert cells.max() > budget
            monkeypatch.setenv("BAMSIGNALS_RUNS_BLOCK_CELLS", str(budget))
            many = call(lower)
            assert "1 GPU slot(s)" in last_call_route() and _blocks(last_call_route()) >= 10
            vx.same_views(_fields(many), want)
            monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
            four = call(lower)
            assert "4 GPU slot(s)" in last_call_route() and _blocks(last_call_route()) >= 10
            vx.same_views(_fields(four), want)
            monkeypatch.delenv("BAMSIGNALS_RUNS_BLOCK_CELLS", raising=False)
            four = call(lower)
            assert "4 GPU slot(s)" in last_call_route() and _blocks(last_call_route()) == 4
            vx.same_views(_fields(four), want)
    finally:
        _lib.load().bsig_cache_clear()


def test_ranges_of_one_base_all_covered(fixture_reads, monkeypatch):
    """ranges of width 1 on covered bases (SNP positions): every segment is one in-cell, as many views as cells"""
    from bamsignals_amd import GRanges, _lib, bamViews
    from oracle import oracle_c
    fx = fixture_reads
    names = [str(s) for s in fx["ref_names"]]
    rid = np.repeat(np.arange(len(names)), np.diff(fx["ref_off"])).astype(I32)[::97][:300]
    loc = ((fx["bam_pos"].astype(np.int64) + fx["bam_end"]) // 2)[::97][:300].astype(I32)      # the middle of a read
    rg = dict(rid=rid, loc=loc, len=np.ones(len(rid), I32), strand=np.zeros(len(rid), I32))
    gr = GRanges([names[r] for r in rid], loc + 1, width=rg["len"], strand=["*"] * len(rid))
    orc = oracle_c.OracleReads(fx["ref_off"], fx["bam_pos"], fx["bam_end"], fx["bam_flag"], fx["bam_mapq"], fx["bam_tlen"])
    flat, off = oracle_c.coverage_core(orc, rg)
    want = vx.views_of_segments(vx.flat_segments(flat, off, False), 1)
    assert len(want[1]) > (len(flat) + 1) // 2                  # more views than one per two cells
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        vx.same_views(_fields(bamViews(BAM, gr, 1, verbose=False)), want)
        both = bamViews(BAM, gr, 1, ss=True, verbose=False)    # one bin per row
        assert both.ss and np.array_equal(both.counts().sum(axis=0) >= 1, np.diff(want[0]) == 1)
    finally:
        _lib.load().bsig_cache_clear()


# ---- file level: the fixture BAM against the goldens -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_gr(fixture_regions):
    from bamsignals_amd import GRanges
    reg, ranges = fixture_regions
    return GRanges(reg["chrom"], reg["start"], width=reg["width"], strand=reg["strand"]), ranges


def test_file_level_against_the_goldens(golden_gr, expected_grid, tmp_path, monkeypatch):
    from bamsignals_amd import _lib, bamCoverage, bamViews
    from bamsignals_amd.wrappers import last_call_route
    from oracle import oracle_c
    gr, ranges = golden_gr
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    monkeypatch.delenv("BAMSIGNALS_DEVICES", raising=False)
    monkeypatch.delenv("BAMSIGNALS_RUNS_BLOCK_CELLS", raising=False)
    _lib.load().bsig_cache_clear()
    try:
        # coverage at 2 and above
        golden = expected_grid["coverage|mapq=0,pe=ignore,tf=NULL"]
        off = oracle_c.layout(ranges["len"], 1, False)
        segs = vx.flat_segments(golden, off, False)
        sig = bamViews(BAM, gr, 2, verbose=False)
        assert "views of 1 block(s)" in last_call_route() and not sig.ss and len(sig) == len(gr)
        vx.same_views(_fields(sig), vx.views_of_segments(segs, 2))
        vx.check_invariants(_fields(sig), segs, 2)
        assert sig.nviews > len(gr)
        # ... a band, and a depth nothing reaches
        band = bamViews(BAM, gr, 1, 2, verbose=False)
        vx.same_views(_fields(band), vx.views_of_segments(segs, 1, 2))
        none = bamViews(BAM, gr, int(golden.max()) + 1, verbose=False)
        assert none.nviews == 0 and not none.seg_off.any() and len(none) == len(gr)
        # its BED against lines made per bin from the golden vectors
        path = tmp_path / "views.bed"
        assert sig.to_bed(path, gr) == sig.nviews
        want = []
        for i in range(len(gr)):
            want += vx.lines_per_bin(segs[i], gr.seqnames[i], gr.start[i], gr.width[i], gr.strand[i], i, 2)
        assert open(path).read().splitlines() == want
        # at 1 and above: the non-zero runs of the run-length coverage, joined (an extra assertion, not the expectation)
        at1 = bamViews(BAM, gr, 1, verbose=False)
        vx.same_views(_fields(at1), vx.views_of_segments(segs, 1))
        runs = bamCoverage(BAM, gr, runs=True, verbose=False)
        for i in range(len(gr)):
            values, lengths = runs[i]
            end = np.cumsum(lengths, dtype=np.int64)
            nz = values != 0
            first = nz & ~np.concatenate([[False], nz[:-1]])
            last = nz & ~np.concatenate([nz[1:], [False]])
            assert np.array_equal(at1[i]["start"], (end - lengths)[first]) and np.array_equal(at1[i]["start"] + at1[i]["width"], end[last])
        # the 5' ends, strand-specific, at 1 and above; with bins of 7 its BED per bin
        golden = expected_grid["profile|shift=0,mapq=0,ss=1,pe=ignore,tf=NULL"]
        off = oracle_c.layout(ranges["len"], 1, True)
        segs = vx.flat_segments(golden, off, True)
        sig = bamViews(BAM, gr, 1, signal="ends", ss=True, verbose=False)
        assert sig.ss and len(sig) == len(gr) and "views" in last_call_route()
        vx.same_views(_fields(sig), vx.views_of_segments(segs, 1))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                     # (widths that 7 does not divide)
            binned = bamViews(BAM, gr, 2, signal="ends", ss=True, binsize=7, verbose=False)
        for row in (0, 1):
            bins = [np.add.reduceat(s.astype(np.int64), np.arange(0, len(s), 7)) if len(s) else s for s in segs[row::2]]
            assert binned.to_bed(path, gr, binsize=7, row=row) == int(binned.counts()[row].sum())
            want = []
            for i in range(len(gr)):
                want += vx.lines_per_bin(bins[i], gr.seqnames[i], gr.start[i], gr.width[i], gr.strand[i], i, 2, binsize=7)
            assert open(path).read().splitlines() == want and len(want) > 0
    finally:
        _lib.load().bsig_cache_clear()
