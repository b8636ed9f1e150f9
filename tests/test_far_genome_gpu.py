"""GPU: every query kind on decks that lie far out in the genome -- past cumulative 2^32 and 2^36 bp, across 2^32, around
base 2^30 of a reference and 1,000 bases below base 2^31 - 1 (tests/far_deck.py: the placements).

The resident layout addresses a read by ``g = (ref_unit0 << 16) + pos``; the suite's other decks stay below g = 2^24 and
tests/test_large_genome_gpu.py below 2^32, with three kinds.  A kernel's cost depends on the reads, not on the genome, so the
small decks the suite trusts are moved: tests/forms_deck.py (140k reads; the default layout and BAMSIGNALS_PACK=0) to the
five named placements, the spliced, junction and gene-count decks to those and to six more that put 2^k and 2^k + 1
references in front of the sorts' ``reference << 32 | start`` keys.  The expected side of every case is computed directly on
the placed columns and ranges by the C oracle and the kinds' restatements; tests/test_far_deck_cpu.py proves without a GPU
that it equals the near one moved by D and that no case is vacuous.  Every comparison is exact, every result non-zero; a
mismatch names the references whose ranges differ.  No kernel form is chosen by environment: the forms matrices do that
where the deck is; this module is about where the reads lie.  Every plan runs twice, as in the forms tests: the first run
looks its windows up, the second reads the kept ones.

The later kinds' parameter sets are taken from their own forms tests and named in LATER_KINDS.

Plan statistics: the per-class reads in the tiles' exact index windows (class_window in k_resolve and k_visits, which also
size a plan's heavy tiles) are compared with the near plan's, because no result on this deck depends on them.

Measured on an MI355X: 459 cases in 28.5 s of wall time for the whole module, the expected sides included; the slowest
case (the cross-correlation's expected side) takes 1.0 s, making the first resident set 1.7 s.

What it found (profiles/far_genome.md): at every placement every kind agrees with its expected side -- no 32-bit slip.
The clone cases failed for a reason that does not depend on the placement: bsig_reads_clone left the clone's layout
number at 0, so a plan's second run on a clone took its tiles' windows for looked up already and read a table nothing
had written (fixed in csrc/runtime.hip)."""
import functools
import itertools

import numpy as np
import pytest

import far_deck as fd
import forms_deck as deck

pytestmark = pytest.mark.gpu

FILTERS = (dict(), dict(mapqual=30, filteredF=0x400))           # tests/test_junctions_gpu.py: FILTERS
ANCHORS = (0, 8)
JUNCTION_TABLES = ("whole", "tiles", "genes")
# spliced coverage (binsize, ss, filter): per range, binned with strands, and binned with strands under a filter
COVERAGE_SETS = ((1, False, {}), (7, True, {}), (200, True, dict(mapqual=30, filteredF=0x400)))
HANGING_RANGES = [2, 5, 6]          # forms_deck.ranges(): loc = -3
HANGING_SUM_RANGES = [0]            # forms_deck.sum_ranges(): loc = -5
FORMS_LAYOUTS = {"packed": None, "nopack": "0"}                 # BAMSIGNALS_PACK

# The later kinds, one parameter set each, with where it comes from:
#   xcorr          test_reduction_forms_gpu.XCORR[3]: max_lag 200, bodies of 2,048 cells
#   frag           test_reduction_forms_gpu.FRAG, FRAG_SHAPES[1]: tlen 100 .. 400 in bins of 7, the midpoint rule
#   hist_cover     test_reduction_forms_gpu.TILES[0] x HIST: coverage, tiles of 18 cells, max_value 50
#   hist_ends      TILES[5] x HIST: 5' ends with strands, tiles of 2,048 cells, max_value 50
#   summary        TILES[5] x SUMMARY: 5' ends with strands, the eight thresholds
#   scaled         TILES[0] x SCALED: coverage in 20 bins a range
#   overlap_any / overlap_within   test_overlaps_gpu.DECK_SETS "plain" / "extend", minoverlap DECK_M = 5
#   resized / resized_sum          test_later_forms_gpu: frag_len RESIZED_L[0] = 36 on bins2_ss1 (64-cell tiles) and on the sum
#   capped_ends    test_later_forms_gpu.CAPPED: keepDup 2, bins of 7 with strands, shift 75, 256-cell tiles
#   capped_cover   test_later_forms_gpu.CAPPED_COVER[1]: keepDup 2, reads resized to 36, bins of 50 with strands
#   vplot          test_later_forms_gpu.VPLOT "small": tlen 0 .. 600 in bins of 7, 50-base columns, the midpoint rule
LATER_KINDS = ("xcorr", "frag", "hist_cover", "hist_ends", "summary", "scaled", "overlap_any", "overlap_within", "resized",
               "resized_sum", "capped_ends", "capped_cover", "vplot")
XCORR_LAG, FRAG_TF, FRAG_BIN, MAX_VALUE, N_BINS, OVERLAP_M, FRAG_LEN, KEEP_DUP, CAPPED_SHIFT = 200, (100, 400), 7, 50, 20, 5, 36, 2, 75
OVERLAP_SETS = {"overlap_any": (False, dict(mapqual=10, ss=True)), "overlap_within": (True, dict(tlen_filter=(0, 400), tspan=True, ss=True))}
VPLOT_TF, VPLOT_LEN_BIN, VPLOT_BINSIZE = deck.VPLOT_SHAPES["small"]
VIEW_LOWER = 5


def parameter_reach():
    """the largest shift, template length and fragment length any parameter set of this module adds to a coordinate"""
    shifts = [a.get("shift", 0) for _, a in list(deck.PARAM_SETS.values()) + list(deck.SUM_SETS.values())] + [CAPPED_SHIFT]
    tlens = [FRAG_TF[1], VPLOT_TF[1]] + [a["tlen_filter"][1] for _, a in OVERLAP_SETS.values() if "tlen_filter" in a]
    return dict(shift=max(shifts), tlen=max(tlens), frag_len=FRAG_LEN)


@functools.lru_cache(maxsize=None)
def _overlap_expected(kind, placement):
    import overlaps_expected as oe
    within, a = OVERLAP_SETS[kind]
    c, rg = (deck.reads(), deck.ranges()) if placement is None else (deck.reads(placement), deck.ranges(placement))
    want = oe.restated(c, rg, within=within, m=OVERLAP_M, **a)
    want.setflags(write=False)
    return want


def later_expected(kind, p):
    """the expected side of a later kind at placement p (None: where the deck is): an array, or (flat, offsets)"""
    if kind == "xcorr":
        return deck.expected_xcorr(XCORR_LAG, 0, placement=p)
    if kind == "frag":
        return deck.expected_frag(FRAG_TF, FRAG_BIN, True, placement=p)
    if kind == "hist_cover":
        return deck.expected_hist("coverage", False, MAX_VALUE, placement=p)
    if kind == "hist_ends":
        return deck.expected_hist("ends", True, MAX_VALUE, placement=p)
    if kind == "summary":
        return deck.expected_summary("ends", True, deck.THRESHOLDS, placement=p)
    if kind == "scaled":
        return deck.expected_scaled("coverage", False, N_BINS, placement=p)
    if kind in OVERLAP_SETS:
        return _overlap_expected(kind, p)
    if kind == "resized":
        return deck.expected_resized(FRAG_LEN, "bins2_ss1", placement=p)
    if kind == "resized_sum":
        return deck.expected_resized_sum(FRAG_LEN, True, placement=p)
    if kind == "capped_ends":
        return deck.expected_capped(KEEP_DUP, 7, True, CAPPED_SHIFT, 0, placement=p)
    if kind == "capped_cover":
        return deck.expected_capped_cover(KEEP_DUP, FRAG_LEN, 50, True, 0, placement=p)
    if kind == "vplot":
        return deck.expected_vplot(VPLOT_TF, VPLOT_LEN_BIN, VPLOT_BINSIZE, True, placement=p)
    raise KeyError(kind)


def later_expected_pairs(p):
    """(kind, near, far) for tests/test_far_deck_cpu.py"""
    for kind in LATER_KINDS:
        yield kind, later_expected(kind, None), later_expected(kind, p)


def later_plan(kind, ctx, reads, p):
    """the plan of a later kind on the placed deck"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import (CappedPlan, FragPlan, HistPlan, Plan, ScaledPlan, SummaryPlan, SumPlan, VplotPlan, XcorrPlan,
                                       make_params)
    rg = deck.sum_ranges(p) if kind in ("resized_sum", "vplot") else deck.ranges(p)
    a = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
    ends = functools.partial(make_params, _lib.MODE_PROFILE, binsize=1)
    if kind == "xcorr":
        return XcorrPlan(*a, ends(tile_cells=2048), XCORR_LAG)
    if kind == "frag":
        return FragPlan(*a, make_params(_lib.MODE_COUNT, binsize=-1, requiredF=66, tlen_filter=FRAG_TF, pe_mid=True), FRAG_BIN)
    if kind == "hist_cover":
        return HistPlan(*a, make_params(_lib.MODE_COVERAGE, tile_cells=18), MAX_VALUE)
    if kind == "hist_ends":
        return HistPlan(*a, ends(ss=True, tile_cells=2048), MAX_VALUE)
    if kind == "summary":
        return SummaryPlan(*a, ends(ss=True, tile_cells=2048), deck.THRESHOLDS)
    if kind == "scaled":
        return ScaledPlan(*a, make_params(_lib.MODE_COVERAGE, tile_cells=18), N_BINS)
    if kind in OVERLAP_SETS:
        within, kw = OVERLAP_SETS[kind]
        return Plan(*a, make_params(_lib.MODE_OVERLAP_WITHIN if within else _lib.MODE_OVERLAP_ANY, binsize=OVERLAP_M, **kw))
    if kind == "resized":
        mode, kw = deck.gpu_args("bins2_ss1")
        return Plan(*a, make_params(mode, tile_cells=64, **kw), frag_len=FRAG_LEN)
    if kind == "resized_sum":
        return SumPlan(*a, make_params(_lib.MODE_COVERAGE_EX, binsize=1, ss=True, tile_cells=256), frag_len=FRAG_LEN)
    if kind == "capped_ends":
        return CappedPlan(*a, make_params(_lib.MODE_PROFILE, binsize=7, ss=True, shift=CAPPED_SHIFT, tile_cells=256), KEEP_DUP)
    if kind == "capped_cover":
        return CappedPlan(*a, make_params(_lib.MODE_COVERAGE_EX, binsize=50, ss=True, tile_cells=2048), KEEP_DUP, FRAG_LEN)
    if kind == "vplot":
        return VplotPlan(*a, make_params(_lib.MODE_PROFILE, tlen_filter=VPLOT_TF, pe_mid=True, binsize=VPLOT_BINSIZE, requiredF=66,
                                         tile_cells=2048), VPLOT_LEN_BIN)
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------
# comparing
# ---------------------------------------------------------------------------------------------------------------
def _refs_that_differ(got, want, off, rid):
    """the references whose ranges differ (tests/test_large_genome_gpu.py: _per_reference_mismatch)"""
    return sorted({int(rid[i]) for i in range(len(rid)) if not np.array_equal(got[off[i]:off[i + 1]], want[off[i]:off[i + 1]])})


def _same(got, want, what, off=None, rid=None):
    got, want = np.asarray(got), np.asarray(want)
    assert want.any(), (what, "the expected side is all zero")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        where = _refs_that_differ(got, want, off, rid) if off is not None and got.ndim == 1 else "a reduction over all ranges"
        raise AssertionError((what, "cells that differ:", len(bad), "first:", bad[:8].tolist(), "references:", where))


def _run_twice(plan, want, what, off=None, rid=None):
    try:
        first, second = plan.run_host().copy(), plan.run_host().copy()
    finally:
        plan.close()
    _same(first, want, (what, "first run"), off, rid)
    _same(second, want, (what, "second run"), off, rid)


# ---------------------------------------------------------------------------------------------------------------
# the resident sets
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _upload(ctx, cols, pack=None):
    """a resident set made with BAMSIGNALS_PACK as given (None: the default layout) and no other layout knob"""
    from bamsignals_amd.device import Reads
    mp = pytest.MonkeyPatch()
    try:
        for k in ("BAMSIGNALS_SHORT_HALF", "BAMSIGNALS_PACK", "BAMSIGNALS_PACKED_HALF", "BAMSIGNALS_BUCKET_READS"):
            mp.delenv(k, raising=False)
        if pack is not None:
            mp.setenv("BAMSIGNALS_PACK", pack)
        if "cigar" in cols:
            return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                         cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=True)
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    finally:
        mp.undo()


@pytest.fixture(scope="module", params=[(n, lay) for n in fd.FIVE for lay in FORMS_LAYOUTS], ids=lambda v: f"{v[0]}-{v[1]}")
def forms(request, ctx):
    """(context, the placed forms deck resident in one layout, its placement): one set per (placement, layout), closed when
    the module has run its cases"""
    name, layout = request.param
    p = deck.named_placement(name)
    reads = _upload(ctx, deck.reads(p), FORMS_LAYOUTS[layout])
    try:
        info = reads.info()
        assert info["n_reads"] == len(deck.reads()["pos"])
        # a read's class does not depend on where its reference lies
        assert list(info["class_n"][:5]) == np.bincount(deck.read_classes(layout == "packed"), minlength=5).tolist()
        yield ctx, reads, p
    finally:
        reads.close()


@pytest.fixture(scope="module")
def near_forms(ctx):
    """the forms deck where the suite has it, in both layouts: the near side of the plan statistics"""
    out = {layout: _upload(ctx, deck.reads(), pack) for layout, pack in FORMS_LAYOUTS.items()}
    yield out
    for r in out.values():
        r.close()


class _Sets:
    """the resident spliced sets and gene models of one placement (None: the decks where they are), made when first asked for"""

    def __init__(self, ctx, name):
        self.ctx, self.name, self._reads, self._models = ctx, name, {}, {}

    def cols(self, which):
        return fd.near(which).cols if self.name is None else fd.far(which, self.name).cols

    def table(self, which, table):
        return fd.near(which).tables[table] if self.name is None else fd.far(which, self.name).tables[table]

    def reads(self, which):
        if which not in self._reads:
            self._reads[which] = _upload(self.ctx, self.cols(which))
        return self._reads[which]

    def model(self, which):
        from bamsignals_amd import GeneModel
        if which not in self._models:
            ann = fd.near(which).ann
            f = ann.features if self.name is None else fd.far(which, self.name).features
            self._models[which] = GeneModel.from_arrays(f["rid"], f["loc"], f["len"], f["strand"], ann.gene, ann.n_genes,
                                                        len(self.cols(which)["ref_len"]), genes=ann.labels)
        return self._models[which]

    def close(self):
        for x in list(self._reads.values()) + list(self._models.values()):
            x.close()
        self._reads, self._models = {}, {}


@pytest.fixture(scope="module")
def near_sets(ctx):
    s = _Sets(ctx, None)
    yield s
    s.close()


@pytest.fixture(scope="module", params=fd.ELEVEN)
def far_sets(request, ctx):
    s = _Sets(ctx, request.param)
    yield s
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# the forms deck
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", list(deck.PARAM_SETS))
def test_forms_per_range(forms, pset):
    from bamsignals_amd.device import Plan, make_params
    ctx, reads, p = forms
    rg = deck.ranges(p)
    want, off = deck.expected(pset, p)
    mode, a = deck.gpu_args(pset)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(mode, **a))
    assert np.array_equal(plan.offsets, off)
    _run_twice(plan, want, (p.name, pset), off, rg["rid"])


@pytest.mark.parametrize("sset", list(deck.SUM_SETS))
def test_forms_sums(forms, sset):
    from bamsignals_amd.device import SumPlan, make_params
    ctx, reads, p = forms
    rg = deck.sum_ranges(p)
    mode, a = deck.gpu_args(sset)
    _run_twice(SumPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(mode, **a)), deck.expected_sum(sset, p), (p.name, sset))


@pytest.mark.parametrize("kind", LATER_KINDS)
def test_forms_later_kinds(forms, kind):
    ctx, reads, p = forms
    want = later_expected(kind, p)
    off = None
    if isinstance(want, tuple):
        want, off = want
    elif kind in OVERLAP_SETS:                                      # (sense, antisense) per range
        off = 2 * np.arange(len(deck.ranges(p)["rid"]) + 1)
    _run_twice(later_plan(kind, ctx, reads, p), want, (p.name, kind), off, deck.ranges(p)["rid"])


# what a plan says about its tiles' index windows and does not depend on the bucket widths, which follow the genome's size
STAT_KEYS = ("n_items", "cells", "visits", "visits_short", "visits_packed", "heavy_tiles")


@pytest.mark.parametrize("pset", ["word_ss1", "count", "cover", "bins274_ss1"])
def test_forms_plan_statistics_are_the_near_plans(forms, near_forms, pset):
    """The reads in the exact candidate windows of all tiles, counted through the index (class_window, the packed class's
    chunks) when the plan is made: the near plan's, read for read.  Plan creation sizes its heavy tiles by the same
    windows, so a window that came out empty far out would go unnoticed by every result until a tile is deep enough to
    need slicing."""
    from bamsignals_amd.device import Plan, make_params
    ctx, reads, p = forms
    layout = "nopack" if reads.info()["class_n"][4] == 0 else "packed"
    mode, a = deck.gpu_args(pset)
    got = []
    for r, rg in ((reads, deck.ranges(p)), (near_forms[layout], deck.ranges())):
        plan = Plan(ctx, r, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(mode, **a))
        try:
            st = plan.stats()
            got.append({k: int(st[k]) for k in STAT_KEYS})
        finally:
            plan.close()
    far, near = got
    assert far == near, (p.name, pset, far, near)
    assert far["visits"] > far["visits_short"] + far["visits_packed"] > 0           # the long classes too
    assert (far["visits_packed"] > 0) == (layout == "packed")


def test_a_plan_runs_twice_on_a_clone_of_the_forms_deck(forms):
    """a clone is a layout of its own: the second run of a plan on it looks its windows up like the first run on any set"""
    from bamsignals_amd.device import Plan, make_params
    ctx, reads, p = forms
    clone = reads.clone(ctx)
    try:
        rg = deck.ranges(p)
        want, off = deck.expected("word_ss1", p)
        mode, a = deck.gpu_args("word_ss1")
        _run_twice(Plan(ctx, clone, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(mode, **a)), want, (p.name, "clone"), off, rg["rid"])
    finally:
        clone.close()


def test_forms_runs_and_views(forms):
    """runs() and views() of the per-base coverage plan: every run and every view of every range, from the oracle's cells"""
    import torch

    import runs_expected as rn
    import views_expected as vw
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, reads, p = forms
    rg = deck.ranges(p)
    want, off = deck.expected("cover", p)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE))
    enc = ve = None
    try:
        buf = torch.empty(max(plan.cells, 4), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        plan.run_device(buf.data_ptr())
        ctx.sync()
        enc, ve = plan.runs(), plan.views()
        want_runs = rn.encode_many(want, rg["len"])
        assert enc.encode(buf.data_ptr()) == len(want_runs[1]) > 0
        rn.same_runs(enc.fetch(), want_runs)
        want_views = vw.views_of_many(want, rg["len"], VIEW_LOWER)
        assert ve.encode(buf.data_ptr(), VIEW_LOWER) == len(want_views[1]) > 0
        vw.same_views(ve.fetch(), want_views)
    finally:
        for x in (enc, ve, plan):
            if x is not None:
                x.close()


# ---------------------------------------------------------------------------------------------------------------
# the spliced decks
# ---------------------------------------------------------------------------------------------------------------
def _coverage_params(binsize, ss, flt):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    if binsize == 1 and not ss and not flt:
        return make_params(_lib.MODE_COVERAGE)
    return make_params(_lib.MODE_COVERAGE_EX, binsize=binsize, ss=ss, **flt)


def _check_coverage(ctx, reads, b, rg, what):
    """the spliced coverage of a set: per range, binned with strands, under a filter; the sum; runs and views"""
    import torch

    import runs_expected as rn
    import spliced_expected as sx
    import views_expected as vw
    from bamsignals_amd.device import Plan, SumPlan
    a = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
    for binsize, ss, flt in COVERAGE_SETS:
        plan = Plan(*a, _coverage_params(binsize, ss, flt))
        off = np.asarray(plan.offsets).copy()
        _run_twice(plan, sx.expected_coverage(b, rg, binsize=binsize, ss=ss, **flt), (what, binsize, ss, flt), off, rg["rid"])
    assert len(set(rg["len"].tolist())) == 1                        # a tiling of whole multiples: one width, as a sum needs
    want = sx.expected_coverage(b, rg, binsize=10, ss=True)
    prm = _coverage_params(10, True, {})
    _run_twice(SumPlan(*a, prm), want.reshape(len(rg["rid"]), -1).astype(np.int64).sum(axis=0), (what, "sum"))
    plan = Plan(*a, prm)
    enc = ve = None
    try:
        buf = torch.empty(max(plan.cells, 4), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        plan.run_device(buf.data_ptr())
        ctx.sync()
        segs = rn.flat_segments(want, plan.offsets, True)          # segment 2 i + antisense
        enc, ve = plan.runs(), plan.views()
        want_runs = rn.encode_segments(segs)
        assert enc.encode(buf.data_ptr()) == len(want_runs[1]) > 0
        rn.same_runs(enc.fetch(), want_runs)
        want_views = vw.views_of_segments(segs, VIEW_LOWER)
        assert ve.encode(buf.data_ptr(), VIEW_LOWER) == len(want_views[1]) > 0
        vw.same_views(ve.fetch(), want_views)
    finally:
        for x in (enc, ve, plan):
            if x is not None:
                x.close()


@pytest.mark.parametrize("which", ["hand", "random"])
def test_spliced_coverage(ctx, near_sets, far_sets, which):
    reads, near = far_sets.reads(which), near_sets.reads(which)
    b = fd.blocks(which, far_sets.name)
    assert reads.spliced and reads.info()["n_reads"] == near.info()["n_reads"] == len(b["pos"])
    assert reads.n_source_reads == near.n_source_reads == len(far_sets.cols(which)["pos"])
    _check_coverage(ctx, reads, b, far_sets.table(which, "tiles"), (far_sets.name, which))


def _query(reads, rg, **kw):
    return reads.junctions(rg["rid"], rg["loc"], rg["len"], rg["strand"], **kw)


def _junction_refs_that_differ(got, want, rid):
    """the references of the ranges whose junctions differ"""
    bad = set()
    for i in range(len(rid)):
        (a, b), (c, d) = got[0][i:i + 2], want[0][i:i + 2]
        if b - a != d - c or any(not np.array_equal(np.asarray(got[k])[a:b], np.asarray(want[k])[c:d]) for k in (1, 2, 3, 4)):
            bad.add(int(rid[i]))
    return sorted(bad)


@pytest.mark.parametrize("which", fd.SPLICED_DECKS)
def test_junctions(near_sets, far_sets, which):
    import junctions_expected as jx
    reads, near = far_sets.reads(which), near_sets.reads(which)
    p = fd.far(which, far_sets.name).placement
    jr = fd.junction_rows(which, far_sets.name)
    assert reads.n_junction_rows == near.n_junction_rows == len(jr["start"]) > 0
    seen = 0
    for table, ss, flt, anchor in itertools.product(JUNCTION_TABLES, (False, True), FILTERS, ANCHORS):
        rg, rg0 = far_sets.table(which, table), near_sets.table(which, table)
        want = jx.expected(jr, rg, ss=ss, min_anchor=anchor, **flt)
        got = _query(reads, rg, ss=ss, min_anchor=anchor, **flt)
        what = (p.name, which, table, ss, flt, anchor)
        assert len(got) == 5 and len(got[0]) == len(want[0]), what
        assert jx.same(got, want), (what, "references:", _junction_refs_that_differ(got, want, rg["rid"]))
        # start - D, end - D, the counts, the anchors and seg_off are the near set's
        assert jx.same(fd.unplace_junctions(got, p), _query(near, rg0, ss=ss, min_anchor=anchor, **flt)), what
        seen += int(want[0][-1])
    assert seen > 0


@pytest.mark.parametrize("which", list(fd.GENE_DECKS))
def test_gene_counts(near_sets, far_sets, which):
    import genecounts_expected as gx
    reads, model = far_sets.reads(which), far_sets.model(which)
    near, near_model = near_sets.reads(which), near_sets.model(which)
    far, ann = fd.far(which, far_sets.name), fd.near(which).ann
    for mode, flt in itertools.product(gx.MODES, FILTERS):
        counts, summary = reads.gene_counts(model, strand=mode, **flt)
        want_counts, want_summary = gx.expected(far.cols, far.features, ann.gene, ann.n_genes, strand=mode, **flt)
        what = (far_sets.name, which, mode, flt)
        assert want_summary[0] > 0 and counts.dtype == summary.dtype == np.int64
        if not np.array_equal(counts, want_counts):
            genes = np.flatnonzero(counts != want_counts)
            refs = sorted(set(far.features["rid"][np.isin(ann.gene, genes)].tolist()))
            raise AssertionError((what, "genes that differ:", genes[:8].tolist(), "references:", refs))
        assert np.array_equal(summary, want_summary), (what, summary, want_summary)
        near_counts, near_summary = near.gene_counts(near_model, strand=mode, **flt)
        assert np.array_equal(counts, near_counts) and np.array_equal(summary, near_summary), what


def test_a_clone_answers_the_same(ctx, far_sets):
    """a clone of the far junction set: coverage, junctions and gene counts"""
    import genecounts_expected as gx
    import junctions_expected as jx
    which = "junction"
    clone = far_sets.reads(which).clone(ctx)
    try:
        b, jr = fd.blocks(which, far_sets.name), fd.junction_rows(which, far_sets.name)
        assert clone.spliced and clone.info()["n_reads"] == len(b["pos"]) and clone.n_junction_rows == len(jr["start"])
        _check_coverage(ctx, clone, b, far_sets.table(which, "tiles"), (far_sets.name, "clone"))
        rg = far_sets.table(which, "genes")
        want = jx.expected(jr, rg, ss=True, min_anchor=8, **FILTERS[1])
        got = _query(clone, rg, ss=True, min_anchor=8, **FILTERS[1])
        assert want[0][-1] > 0 and jx.same(got, want), _junction_refs_that_differ(got, want, rg["rid"])
        far, ann = fd.far(which, far_sets.name), fd.near(which).ann
        counts, summary = clone.gene_counts(far_sets.model(which), strand="reverse", **FILTERS[1])
        want_counts, want_summary = gx.expected(far.cols, far.features, ann.gene, ann.n_genes, strand="reverse", **FILTERS[1])
        assert want_summary[0] > 0 and np.array_equal(counts, want_counts) and np.array_equal(summary, want_summary)
    finally:
        clone.close()
