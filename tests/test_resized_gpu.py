"""GPU: bamCoverage of single-end reads resized to the fragment (Plan / SumPlan(frag_len=L), bamCoverage(fragLength=L))
against tests/resized_expected.py -- the project's unchanged oracle coverage on the resized read columns --, exactly.
The forms deck (tests/forms_deck.py) in the packed layout and with every short read in class 0, planted reads at every
edge of a tile's window, the identities with bamProfile and with paired.end = "extend", a tile that is heavy only
because its window was widened, the longest fragment the ABI takes, the sums and runs, the file-level calls, and what
the resized creators refuse."""
import ctypes as C
import os

import numpy as np
import pytest

import forms_deck as deck
import resized_expected as rx
import runs_expected as re_

pytestmark = pytest.mark.gpu

LENGTHS = (1, 36, 200, 257, 5000)
PSETS = ("cover", "bins2_ss0", "bins2_ss1", "bins274_ss1")
LAYOUTS = ("packed", "nopack")
FRAG_LEN_MAX = 1 << 24
ARG = -1


def upload(ctx, cols, pack=True):
    """the columns resident on the GPU: the default layout (short reads of frequent pairs packed), or with
    BAMSIGNALS_PACK=0 every short read in class 0, as tests/test_kernel_forms_gpu.py forces it"""
    from bamsignals_amd.device import Reads
    old = os.environ.get("BAMSIGNALS_PACK")
    try:
        os.environ.pop("BAMSIGNALS_PACK", None)
        if not pack:
            os.environ["BAMSIGNALS_PACK"] = "0"
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    finally:
        os.environ.pop("BAMSIGNALS_PACK", None)
        if old is not None:
            os.environ["BAMSIGNALS_PACK"] = old


@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gpu(ctx):
    """(context, {layout: the deck's Reads})"""
    out = {"packed": upload(ctx, deck.reads()), "nopack": upload(ctx, deck.reads(), pack=False)}
    assert out["packed"].info()["class_n"][4] > 0 and out["nopack"].info()["class_n"][4] == 0
    yield ctx, out
    for r in out.values():
        r.close()


def both_layouts(ctx, cols):
    out = {"packed": upload(ctx, cols), "nopack": upload(ctx, cols, pack=False)}
    assert out["packed"].info()["class_n"][4] > 0 and out["nopack"].info()["class_n"][4] == 0
    return out


def run_twice(ctx, reads, rg, params, frag_len):
    """the plan's first run (windows looked up in the kernel) and its second (the resolved form), and its stats"""
    from bamsignals_amd.device import Plan
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], params, frag_len=frag_len)
    try:
        return plan.run_host().copy(), plan.run_host().copy(), plan.stats(), plan.offsets.copy()
    finally:
        plan.close()


def cov_params(binsize=1, ss=False, **kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    if binsize == 1 and not ss:
        return make_params(_lib.MODE_COVERAGE, **kw)
    return make_params(_lib.MODE_COVERAGE_EX, binsize=binsize, ss=ss, **kw)


# ---- 1. the forms deck -----------------------------------------------------------------------------------------------
deck_resized = deck.resized_columns      # (the deck holds them: tests/test_later_forms_gpu.py compares with the same)
deck_expected = deck.expected_resized


@pytest.mark.parametrize("threads", [64, 128, 256])
@pytest.mark.parametrize("tile", deck.TILES)
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("L", LENGTHS)
def test_forms_deck(gpu, L, layout, pset, tile, threads):
    ctx, reads = gpu
    args = deck.PARAM_SETS[pset][1]
    want, off = deck_expected(L, pset)
    first, second, st, poff = run_twice(ctx, reads[layout], deck.ranges(), cov_params(tile_cells=tile, threads=threads, **args), L)
    assert want.any() and np.array_equal(poff, off)
    assert np.array_equal(first, want), int(np.sum(first != want))
    assert np.array_equal(second, want), int(np.sum(second != want))
    # no tlen column is read for the length: a packed visit is its word
    assert st["bytes_per_visit_packed"] == 4 and st["bytes_per_visit_short"] == 8 and st["bytes_per_visit_long"] == 12
    assert (st["visits_packed"] > 0) == (layout == "packed")


def test_forms_deck_widens_the_windows(gpu):
    """ext = L - 1: a longer fragment can only add reads to a tile's exact window"""
    ctx, reads = gpu
    visits = [run_twice(ctx, reads["packed"], deck.ranges(), cov_params(tile_cells=256), L)[2]["visits"] for L in LENGTHS]
    assert visits == sorted(visits) and visits[0] < visits[-1]


# ---- 2. planted edges ------------------------------------------------------------------------------------------------
EDGE_L = 100
EDGE_REF = 5000


def edge_columns():
    """reads (pos, span, reverse) around the tiles [1000, 1064), [1064, 1128), [1128, 1192) of a range at 1000 (64-cell
    tiles) with L = 100, on one reference of 5,000 bp"""
    L = EDGE_L
    planted = [
        (1064 - L, 30, False),       # forward, last base 1063: one before the second tile's first cell
        (1065 - L, 30, False),       # ... last base 1064: that tile's first cell
        (1128 - L, 30, False),       # ... last base 1127: that tile's last cell
        (1128 + L - 30, 30, True),   # reverse, end 1227, first base 1128: one past the second tile's last cell
        (1127 + L - 30, 30, True),   # ... first base 1127: that tile's last cell
        (1000 - (L - 1), 25, False),  # forward, starts L - 1 before the range: its last base is the range's first
        (1000 - L, 25, False),       # ... starts L before it: ends one base short
        (1050, 150, False),          # longer than L, forward: trimmed to [1050, 1149]
        (1000, 150, True),           # ... reverse: trimmed to [1050, 1149]
        (4950, 40, False),           # forward fragment [4950, 5049]: past the reference's last base 4999
        (4990, 10, True),            # reverse, its end is the last base
        (10, 40, True),              # reverse, end 49: its resized start is -50
        (0, 1, False),               # a one-base read at base 0
        (2000, 256, True), (2100, 255, False), (2200, 1, True),
    ]
    pos = np.asarray([p for p, _, _ in planted], np.int64)
    order = np.argsort(pos, kind="stable")
    span = np.asarray([s for _, s, _ in planted], np.int64)[order]
    rev = np.asarray([r for _, _, r in planted])[order]
    pos = pos[order]
    n = len(pos)
    return dict(ref_len=np.asarray([EDGE_REF], np.int32), ref_off=np.asarray([0, n], np.int64), pos=pos.astype(np.int32),
                end=(pos + span - 1).astype(np.int32), flag=np.where(rev, 16, 0).astype(np.uint16),
                mapq=np.full(n, 30, np.uint8), tlen=np.zeros(n, np.int32))


def edge_ranges():
    rows = [(1000, 192, 1), (1010, 130, -1), (1000, 192, 1),      # three tiles; a '-' range; the first one again
            (4900, 300, 0), (4800, 250, -1),                       # hang over the reference's last base, one of them mirrored
            (0, 64, 1), (1100, 0, 1), (0, 65, -1),                 # at base 0 (the reverse fragment that starts below it); no width
            (936, 129, 1), (1063, 66, 0), (1127, 103, -1), (1900, 300, 1), (2150, 64, -1)]
    rg = dict(rid=np.zeros(len(rows), np.int32), loc=np.asarray([r[0] for r in rows], np.int32),
              len=np.asarray([r[1] for r in rows], np.int32), strand=np.asarray([r[2] for r in rows], np.int32))
    off = np.concatenate([[0], np.cumsum(rg["len"])])
    assert set((off[:-1][rg["len"] > 0] & 3).tolist()) == {0, 1, 2, 3}
    assert all(64 <= w <= 300 for w in rg["len"] if w)
    return rg


def test_planted_edges_expectation_is_the_brute_force():
    cols, rg = edge_columns(), edge_ranges()
    want, off = rx.expected(cols, rg, EDGE_L)
    for i in range(len(rg["len"])):
        lo, hi = int(rg["loc"][i]), int(rg["loc"][i] + rg["len"][i])
        bf = rx.brute_force(cols, 0, lo, hi, EDGE_L)
        assert np.array_equal(want[off[i]:off[i + 1]], bf[::-1] if rg["strand"][i] < 0 else bf), i
    first = want[off[0]:off[1]]
    # the forward fragments that end on 1063 / 1064 / 1127 and the reverse ones that begin on 1127 / 1128 each move the
    # coverage by one at their cell; the read that starts L before the range misses it, the one L - 1 before covers cell 0
    assert first[0] - first[1] == 1 and first[63] - first[64] == 1 and first[64] - first[65] == 1
    assert first[127] - first[126] == 1 and first[128] == first[127]
    assert want[off[3]:off[4]][100:150].tolist() == [1] * 50 and not want[off[3]:off[4]][150:].any()      # the overhang
    assert want[off[5]:off[6]].tolist() == [2] * 50 + [1] * 14      # the reverse fragment [-50, 49] from base 0 on, over [0, 99]


@pytest.mark.parametrize("threads", [64, 256])
@pytest.mark.parametrize("binsize,ss", [(1, False), (1, True), (3, True), (64, False)])
def test_planted_edges(ctx, binsize, ss, threads):
    cols, rg = edge_columns(), edge_ranges()
    want, off = rx.expected(cols, rg, EDGE_L, binsize, ss)
    reads = both_layouts(ctx, cols)
    try:
        for layout in LAYOUTS:
            first, second, st, poff = run_twice(ctx, reads[layout], rg, cov_params(binsize, ss, tile_cells=64, threads=threads), EDGE_L)
            assert np.array_equal(poff, off) and want.any()
            assert np.array_equal(first, want), (layout, np.flatnonzero(first != want)[:8])
            assert np.array_equal(second, want), (layout, np.flatnonzero(second != want)[:8])
            assert st["n_items"] >= 9
    finally:
        for r in reads.values():
            r.close()


# ---- 3. identities on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_length_one_is_the_stranded_profile(gpu, layout):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, reads = gpu
    rg = deck.ranges()
    ends = Plan(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_PROFILE, binsize=1, shift=0, ss=True))
    try:
        want = ends.run_host().copy()
    finally:
        ends.close()
    first, second, _, _ = run_twice(ctx, reads[layout], rg, cov_params(1, True), 1)
    assert want.any() and np.array_equal(first, want) and np.array_equal(second, want)
    assert np.array_equal(want, deck.expected("half_ss1")[0])


@pytest.mark.parametrize("binsize,ss", [(1, False), (2, True)])
def test_constant_template_length_is_extend(ctx, binsize, ss):
    """the paired islands with |tlen| = 180 throughout: paired.end = "extend" and frag_len = 180 cover the same bases"""
    from bamsignals_amd.device import Plan
    c = dict(deck.reads())
    on = np.isin(np.repeat(np.arange(len(c["ref_len"])), np.diff(c["ref_off"])), c["pair_refs"])
    c["tlen"] = np.where(on, np.where((c["flag"] & 16) != 0, -180, 180), c["tlen"]).astype(np.int32)
    rg = deck.ranges()
    keep = np.isin(rg["rid"], c["pair_refs"])
    rg = {k: v[keep] for k, v in rg.items()}
    kw = dict(requiredF=66, tlen_filter=(0, 1000))
    want, off = rx.expected(c, rg, 180, binsize, ss, **kw)
    reads = both_layouts(ctx, c)
    try:
        for layout in LAYOUTS:
            ext = Plan(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"], cov_params(binsize, ss, tspan=True, **kw))
            try:
                extended = ext.run_host().copy()
            finally:
                ext.close()
            first, second, st, _ = run_twice(ctx, reads[layout], rg, cov_params(binsize, ss, **kw), 180)
            assert want.any() and np.array_equal(extended, want)
            assert np.array_equal(first, want) and np.array_equal(second, want)
            assert st["bytes_per_visit_packed"] == 8          # (the filter's tlen column, not the length's)
    finally:
        for r in reads.values():
            r.close()


# ---- 4. a tile that is heavy only because its window was widened -------------------------------------------------------
HEAVY_L = 20_100


def heavy_columns():
    """16,600 forward reads 20 kbp in front of base 100,000 and 16,600 reverse reads 20 kbp behind it, span 50: resized
    to 20,100 all 33,200 of them cover [100,000, 100,064); as they lie none is within 19 kbp of it"""
    m = 16_600
    rng = np.random.default_rng(9)
    fwd, rev = np.sort(rng.integers(80_000, 80_040, m)), np.sort(rng.integers(120_000, 120_040, m))
    pos = np.concatenate([fwd, rev])
    return dict(ref_len=np.asarray([200_000], np.int32), ref_off=np.asarray([0, 2 * m], np.int64), pos=pos.astype(np.int32),
                end=(pos + 49).astype(np.int32), flag=np.concatenate([np.zeros(m), np.full(m, 16)]).astype(np.uint16),
                mapq=np.full(2 * m, 30, np.uint8), tlen=np.zeros(2 * m, np.int32))


@pytest.mark.parametrize("binsize,ss", [(1, False), (4, True)])
def test_heavy_tile_by_widening(ctx, binsize, ss):
    cols = heavy_columns()
    rg = dict(rid=np.zeros(3, np.int32), loc=np.asarray([100_000, 99_990, 60_000], np.int32), len=np.asarray([64, 100, 64], np.int32),
              strand=np.asarray([1, -1, 0], np.int32))
    want, off = rx.expected(cols, rg, HEAVY_L, binsize, ss)
    assert int(want.reshape(-1, 2).sum(axis=1).max() if ss else want.max()) == 33_200 * binsize
    reads = both_layouts(ctx, cols)
    try:
        for layout in LAYOUTS:
            plain = run_twice(ctx, reads[layout], rg, cov_params(binsize, ss, tile_cells=64), 0)
            assert plain[2]["heavy_tiles"] == 0 and not plain[0][off[0]:off[2]].any()       # as they lie: no read near, none heavy
            first, second, st, _ = run_twice(ctx, reads[layout], rg, cov_params(binsize, ss, tile_cells=64), HEAVY_L)
            assert st["heavy_tiles"] > 0
            assert np.array_equal(first, want), (layout, np.flatnonzero(first != want)[:8])
            assert np.array_equal(second, want), (layout, np.flatnonzero(second != want)[:8])
    finally:
        for r in reads.values():
            r.close()


# ---- 5. the longest fragment -----------------------------------------------------------------------------------------
def test_the_cap(ctx):
    """frag_len = BSIG_FRAG_LEN_MAX on one reference of 40 Mbp: ranges around every fragment's far end, 16.7 Mbp from its
    read, and one 2-Mbp range"""
    L, ref = FRAG_LEN_MAX, 40_000_000
    rng = np.random.default_rng(24)
    n = 300
    pos = np.sort(rng.integers(0, ref - 300, n))
    span = rng.integers(1, 257, n)
    span[::50] = rng.integers(300, 5000, len(span[::50]))
    rev = rng.random(n) < 0.5
    cols = dict(ref_len=np.asarray([ref], np.int32), ref_off=np.asarray([0, n], np.int64), pos=pos.astype(np.int32),
                end=(pos + span - 1).astype(np.int32), flag=np.where(rev, 16, 0).astype(np.uint16),
                mapq=np.full(n, 30, np.uint8), tlen=np.zeros(n, np.int32))
    far = np.where(rev, pos + span - 1 - (L - 1), pos + L - 1)
    loc = np.concatenate([far - 750, [19_000_000]])
    rg = dict(rid=np.zeros(n + 1, np.int32), loc=loc.astype(np.int32), len=np.concatenate([np.full(n, 1500), [2_000_000]]).astype(np.int32),
              strand=rng.choice(np.asarray([1, -1, 0], np.int32), n + 1))
    assert (far < 0).any() and (far >= ref).any() and ((far >= 0) & (far < ref)).any()
    reads = both_layouts(ctx, cols)
    try:
        for binsize, ss in ((1, False), (50, True)):
            want, off = rx.expected(cols, rg, L, binsize, ss)
            for layout in LAYOUTS:
                first, second, _, poff = run_twice(ctx, reads[layout], rg, cov_params(binsize, ss), L)
                assert want.any() and np.array_equal(poff, off)
                assert np.array_equal(first, want), (layout, binsize, np.flatnonzero(first != want)[:8])
                assert np.array_equal(second, want), (layout, binsize)
    finally:
        for r in reads.values():
            r.close()


# ---- 6. sums and runs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [36, 5000])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sum_over_ranges(gpu, layout, ss, L):
    from bamsignals_amd.device import SumPlan
    ctx, reads = gpu
    rg = deck.sum_ranges()
    per_range, _ = rx.coverage(deck_resized(L), rg, 1, ss)
    want = per_range.reshape(len(rg["len"]), -1).sum(axis=0)
    for nw in (1, 4):
        plan = SumPlan(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"], cov_params(1, ss, tile_cells=256, threads=64 * nw),
                       frag_len=L)
        try:
            first, second = plan.run_host().copy(), plan.run_host().copy()
        finally:
            plan.close()
        assert want.any() and first.dtype == np.int64
        assert np.array_equal(first, want) and np.array_equal(second, want)


@pytest.mark.parametrize("pset", ["cover", "bins2_ss1"])
def test_runs_of_a_resized_plan(gpu, pset):
    import torch
    from bamsignals_amd.device import Plan
    ctx, reads = gpu
    args = deck.PARAM_SETS[pset][1]
    rg = deck.ranges()
    want, off = deck_expected(200, pset)
    plan = Plan(ctx, reads["packed"], rg["rid"], rg["loc"], rg["len"], rg["strand"], cov_params(**args), frag_len=200)
    enc = plan.runs()
    try:
        buf = torch.empty(max(plan.cells, 4), dtype=torch.int32, device="cuda:0")
        buf.fill_(-7)
        torch.cuda.synchronize()
        plan.run_device(buf.data_ptr())
        ctx.sync()
        assert not plan.overflowed()
        enc.encode(buf.data_ptr())
        got = enc.fetch()
    finally:
        enc.close()
        plan.close()
    segs = re_.flat_segments(want, off, args["ss"])
    re_.check_invariants(*got, segs)
    re_.same_runs(got, re_.encode_segments(segs))


# ---- 7. file level ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deck_bam(tmp_path_factory):
    from bamsignals_amd import GRanges, _lib
    from bamsignals_amd.bamio import write_columns_as_bam
    c = deck.reads()
    names = ["ref%d" % i for i in range(len(c["ref_len"]))]
    path = str(tmp_path_factory.mktemp("resized") / "deck.bam")
    cig = dict(cigar_off=np.arange(len(c["pos"]) + 1, dtype=np.int64),
               cigar=((c["end"].astype(np.int64) - c["pos"] + 1) << 4).astype(np.uint32))
    write_columns_as_bam(path, names, dict(c, **cig))
    # what the file holds: a read flagged unmapped ends where it starts, whatever its CIGAR says (bam_endpos)
    from oracle import oracle_c
    cols = dict(c, end=oracle_c.cigar_end(c["pos"], c["flag"], cig["cigar_off"], cig["cigar"]))
    assert 0 < int(np.sum(cols["end"] != c["end"])) == int(np.sum(((c["flag"] & 4) != 0) & (c["end"] != c["pos"])))

    def granges(rg):
        return GRanges([names[r] for r in rg["rid"]], rg["loc"].astype(np.int64) + 1, width=rg["len"],
                       strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in rg["strand"]])
    yield path, granges, cols
    _lib.load().bsig_cache_clear()


def _flat(signals, ss):
    return np.concatenate([np.asarray(s).T.reshape(-1) if ss else np.asarray(s) for s in signals])


def test_file_level(deck_bam):
    import warnings
    from bamsignals_amd import bamCoverage
    path, granges, cols = deck_bam
    rg = deck.ranges()
    want, off = rx.expected(cols, rg, 200, 5, True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (widths that are no multiple of the binsize)
        sig = bamCoverage(path, granges(rg), fragLength=200, binsize=5, ss=True, verbose=False)
        runs = bamCoverage(path, granges(rg), fragLength=200, binsize=5, ss=True, runs=True, verbose=False)
    assert want.any() and np.array_equal(_flat(sig, True), want)
    segs = re_.flat_segments(want, off, True)
    re_.same_runs((runs.seg_off, runs.values, runs.lengths), re_.encode_segments(segs))
    # the sum over ranges of one width
    srg = deck.sum_ranges()
    per_range, _ = rx.coverage(rx.resize_columns(cols, 200), srg, 5, True)
    total = per_range.reshape(len(srg["len"]), -1).sum(axis=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        agg = bamCoverage(path, granges(srg), fragLength=200, binsize=5, ss=True, aggregate=True, verbose=False)
    assert agg.dtype == np.int64 and np.array_equal(np.asarray(agg).T.reshape(-1), total)
    # per base and unstranded through the same entry point
    plain = bamCoverage(path, granges(rg), fragLength=200, verbose=False)
    assert np.array_equal(_flat(plain, False), rx.expected(cols, rg, 200)[0])


def test_file_level_without_a_length_is_the_call_it_was(deck_bam):
    from bamsignals_amd import bamCoverage
    path, granges, cols = deck_bam
    rg = deck.ranges()
    none = bamCoverage(path, granges(rg), fragLength=None, verbose=False)
    old = bamCoverage(path, granges(rg), verbose=False)
    assert np.array_equal(_flat(none, False), _flat(old, False))
    assert np.array_equal(_flat(old, False), rx.coverage(cols, rg)[0])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
RANGE_MSG = "the fragment length must be between 1 and 16777216 (%d given)"


def test_refusals(gpu):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, SumPlan, make_params
    ctx, reads = gpu
    rg = deck.sum_ranges()
    r = (ctx, reads["packed"], rg["rid"], rg["loc"], rg["len"], rg["strand"])
    lib = _lib.load()

    def refused(make, message):
        with pytest.raises(_lib.BsigError) as ei:
            make()
        assert ei.value.code_name == "BSIG_ERR_ARG" and str(message) in str(ei.value), str(ei.value)
    for cls in (Plan, SumPlan):
        for mode in (_lib.MODE_PROFILE, _lib.MODE_COUNT, _lib.MODE_OVERLAP_ANY, _lib.MODE_OVERLAP_WITHIN):
            refused(lambda: cls(*r, make_params(mode), frag_len=200),
                    "reads are resized to the fragment for bamCoverage only (mode %d given)" % mode)
        for mode in (_lib.MODE_COVERAGE, _lib.MODE_COVERAGE_EX):
            refused(lambda: cls(*r, make_params(mode, tspan=True, tlen_filter=(0, 1000)), frag_len=200),
                    "a paired-end fragment already has its length: tspan must be 0 with a fragment length")
            for bad in (-1, FRAG_LEN_MAX + 1):
                refused(lambda: cls(*r, make_params(mode), frag_len=bad), RANGE_MSG % bad)
    # a length of 0 (device.Plan's "off") straight at the creators
    n = len(rg["rid"])
    ptrs = [np.ascontiguousarray(rg[k], np.int32) for k in ("rid", "loc", "len", "strand")]
    for name in ("bsig_plan_create_resized", "bsig_plan_create_sum_resized"):
        h = C.c_void_p()
        p = make_params(_lib.MODE_COVERAGE)
        rc = getattr(lib, name)(ctx._h, reads["packed"]._h, n, *[a.ctypes.data for a in ptrs], C.byref(p), 0, C.byref(h))
        assert (rc, lib.bsig_last_error().decode(), h.value) == (ARG, RANGE_MSG % 0, None)
    # the reduction creators refuse what they refused: coverage_ex has no depth histogram, summary or scaled regions; a
    # cross-correlation and a fragment-length histogram are not made of coverage
    from bamsignals_amd.device import FragPlan, HistPlan, ScaledPlan, SummaryPlan, XcorrPlan
    ex = make_params(_lib.MODE_COVERAGE_EX, binsize=2, ss=True)
    refused(lambda: HistPlan(*r, ex, 100), "the depth histogram of coverage is per base and unstranded")
    refused(lambda: SummaryPlan(*r, ex, (1,)), "the range summary of coverage is per base and unstranded")
    refused(lambda: ScaledPlan(*r, ex, 10), "the scaled regions of coverage are per base and unstranded")
    refused(lambda: XcorrPlan(*r, make_params(_lib.MODE_COVERAGE), 100), "the strand cross-correlation is defined on bamProfile")
    refused(lambda: FragPlan(*r, make_params(_lib.MODE_COVERAGE), 1), "the fragment-length histogram is defined on bamCount")
    refused(lambda: SumPlan(*r, make_params(_lib.MODE_COUNT, binsize=-1)), "bamCount has no sum over ranges")
    # ... and an ordinary plan still knows six modes
    refused(lambda: Plan(*r, make_params(6)), "unknown mode 6")
