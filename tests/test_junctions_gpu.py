"""GPU: the junction table of spliced reads and the junction query at handle level (Reads.junctions) and at file level
(bamJunctions), against tests/junctions_expected.py: the numpy restatement of the rows, their anchors and the per-range
result.  All results are integers and compared exactly."""
import itertools

import numpy as np
import pytest

import junctions_expected as jx
import spliced_expected as sx
from bamsignals_amd import GRanges, _lib, bamCoverage, bamJunctions
from bamsignals_amd.bamio import write_columns_as_bam
from bamsignals_amd.device import Context, Plan, Reads, make_params
from bamsignals_amd.synth import synth_reads, tile_ranges
from bamsignals_amd.wrappers import last_call_route, last_call_timing

pytestmark = pytest.mark.gpu

I32 = np.int32
FILTERS = (dict(), dict(mapqual=30, filteredF=0x400))
ANCHORS = (0, 1, 8, 51)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def upload(ctx, cols, spliced=True):
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                 cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=spliced)


@pytest.fixture(scope="module")
def decks(ctx):
    """name -> (CIGAR columns, the restated junction rows, the resident spliced set): made once, shared, left unchanged"""
    out = {}
    for name, cols in (("junction", jx.junction_deck()), ("hand", sx.hand_deck()), ("random", sx.random_deck())):
        out[name] = (cols, jx.rows(cols), upload(ctx, cols))
    yield out
    for _, _, reads in out.values():
        reads.close()


def ranges(rid, loc, ln, strand):
    return dict(rid=np.asarray(rid, I32), loc=np.asarray(loc, I32), len=np.asarray(ln, I32), strand=np.asarray(strand, I32))


def whole_references(cols):
    n = len(cols["ref_len"])
    return ranges(np.arange(n), np.zeros(n), cols["ref_len"], np.zeros(n))


def tiling(cols):
    rg = tile_ranges(cols["ref_len"], 5000)
    rg["strand"] = (np.arange(len(rg["rid"])) % 3 - 1).astype(I32)       # - * + cycling
    return rg


def feature_ranges(name, cols, jr):
    """the deck's genes; for the decks without genes, every 40th junction with 5 bases on either side"""
    if name == "junction":
        return jx.junction_genes()
    k = np.arange(0, len(jr["start"]), 40)
    return ranges(jr["ref"][k], jr["start"][k] - 5, jr["end"][k] - jr["start"][k] + 11, np.arange(len(k)) % 3 - 1)


def twice_and_reversed(rg):
    return {k: np.concatenate([v, v, v[::-1]]) for k, v in rg.items()}


def query(reads, rg, **kw):
    return reads.junctions(rg["rid"], rg["loc"], rg["len"], rg["strand"], **kw)


# ---- the table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck", ["junction", "hand", "random"])
def test_table(ctx, decks, deck):
    cols, jr, reads = decks[deck]
    assert reads.spliced and reads.n_junction_rows == len(jr["start"]) > 0
    rg = whole_references(cols)
    want = jx.expected(jr, rg, ss=True)
    assert jx.same(query(reads, rg, ss=True), want)
    clone = reads.clone(ctx)
    assert clone.n_junction_rows == reads.n_junction_rows and clone.info()["hbm_bytes"] >= 16 * len(jr["start"])
    assert jx.same(query(clone, rg, ss=True), want)
    clone.close()
    plain = upload(ctx, cols, spliced=False)
    assert not plain.spliced and plain.n_junction_rows == 0
    with pytest.raises(_lib.BsigError, match="junctions need spliced reads") as ei:
        query(plain, rg)
    assert ei.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError, match="min_anchor must not be negative"):
        query(reads, rg, min_anchor=-1)
    with pytest.raises(_lib.BsigError, match="range 1 has a negative width"):
        query(reads, ranges([0, 0], [0, 0], [10, -1], [0, 0]))
    with pytest.raises(_lib.BsigError, match="reference 3 is not one of the set's 3"):
        query(reads, ranges([3], [0], [10], [0]))
    plain.close()


# ---- query == restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["references", "tiling", "features", "twice_and_reversed"])
@pytest.mark.parametrize("deck", ["junction", "hand", "random"])
def test_query_is_the_restatement(decks, deck, kind):
    cols, jr, reads = decks[deck]
    rg = dict(references=whole_references, tiling=tiling)[kind](cols) if kind in ("references", "tiling") \
        else feature_ranges(deck, cols, jr)
    if kind == "twice_and_reversed":
        rg = twice_and_reversed(rg)
    seen = 0
    for ss, flt, anchor in itertools.product((False, True), FILTERS, ANCHORS):
        want = jx.expected(jr, rg, ss=ss, min_anchor=anchor, **flt)
        got = query(reads, rg, ss=ss, min_anchor=anchor, **flt)
        assert jx.same(got, want), (ss, flt, anchor)
        assert got[3].dtype == np.uint32 and got[0].dtype == np.int64
        if deck == "junction" and anchor == 51:
            assert not want[0].any(), "reads of 100 bases: every segment is empty"
        seen += int(want[0][-1])
    assert seen > 0


# ---- planted edges ----------------------------------------------------------------------------------------------------------
def heaviest(jr):
    """(ref, start, end, rows) of the deck's junction with the most rows"""
    u, c = jx.multiplicities(jr)
    k = int(np.argmax(c))
    return int(u[k, 0]), int(u[k, 1]), int(u[k, 2]), int(c[k])


def test_range_edges(decks):
    cols, jr, reads = decks["junction"]
    ref, s, e, rows = heaviest(jr)
    assert rows >= 1024
    # last base end - 1, end, end + 1 (start inside, end outside -- inside -- inside); loc = start and start + 1; width-0 ranges
    # between the others
    rg = ranges([ref] * 9, [s - 10, 0, s - 10, s - 10, s, 0, s + 1, s, s],
                [e - 1 - (s - 10) + 1, 0, e - (s - 10) + 1, e + 1 - (s - 10) + 1, e - s + 1, 0, e - s, 0, e - s], [1, 1, -1, 0, 1, -1, 1, 0, 1])
    for ss, flt in itertools.product((False, True), FILTERS):
        want = jx.expected(jr, rg, ss=ss, **flt)
        got = query(reads, rg, ss=ss, **flt)
        assert jx.same(got, want), (ss, flt)
        per = np.diff(got[0])
        holds = [any((got[1][a:b] == s) & (got[2][a:b] == e)) for a, b in zip(got[0][:-1], got[0][1:])]
        assert holds == [False, False, True, True, True, False, False, False, False]
        assert per[1] == per[5] == per[7] == 0
    got = query(reads, ranges([ref], [s], [e - s + 1], [0]))
    k = int(np.flatnonzero((got[1] == s) & (got[2] == e))[0])
    assert got[3][k] == rows and got[4][k] == jr["anchor"][(jr["ref"] == ref) & (jr["start"] == s) & (jr["end"] == e)].max()


def test_no_ranges_and_no_gaps(ctx, decks):
    _, _, reads = decks["junction"]
    for ss in (False, True):
        got = query(reads, ranges([], [], [], []), ss=ss)
        assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:]) and got[3].shape == ((0, 2) if ss else (0,))
    # synth_reads' CIGAR menu has a few N: as they are the reads give the restated junctions, and those without an N none
    cols = synth_reads(20000, [1_000_000, 400_000], seed=11)
    jr = jx.rows(cols)
    with_n = upload(ctx, cols)
    assert with_n.n_junction_rows == len(jr["start"]) > 0
    assert jx.same(query(with_n, tiling(cols), ss=True, min_anchor=8), jx.expected(jr, tiling(cols), ss=True, min_anchor=8))
    with_n.close()
    coff, cig = cols["cigar_off"], cols["cigar"]
    n_before = np.concatenate([[0], np.cumsum((cig & 0xF) == 3)])
    has_n = n_before[coff[1:]] > n_before[coff[:-1]]
    cols = sx.take(cols, np.flatnonzero(~has_n))
    assert len(cols["pos"]) > 15000 and not np.any((cols["cigar"] & 0xF) == 3)
    plain_but_spliced = upload(ctx, cols)
    assert plain_but_spliced.spliced and plain_but_spliced.n_junction_rows == 0
    rg = tiling(cols)
    got = query(plain_but_spliced, rg, ss=True)
    assert got[0].tolist() == [0] * (len(rg["rid"]) + 1) and got[3].shape == (0, 2)
    plain_but_spliced.close()


@pytest.mark.parametrize("at", [63, 64, 255, 256])
def test_run_begins_at_a_chosen_work_item(decks, at):
    """`at` ranges of one row each (a start only one row has) stand in front of a range whose slice opens with a long run of
    equal rows: the run begins at work item `at` of the launch -- the last lane of a wave, the first of the next, the last of
    a workgroup, the first of the next"""
    cols, jr, reads = decks["junction"]
    ref, s, _, _ = heaviest(jr)
    pairs, n = np.unique(np.stack([jr["ref"], jr["start"]], axis=1), axis=0, return_counts=True)
    lone_ref, lone_start = (int(x) for x in pairs[np.flatnonzero(n == 1)[0]])
    run = np.flatnonzero((jr["ref"] == ref) & (jr["start"] == s))
    first_end = int(jr["end"][run[0]])
    run_len = int(np.count_nonzero(jr["end"][run] == first_end))
    assert run_len >= 257, "the run crosses a workgroup"
    hi = int(jr["end"][run].max()) + 3
    rg = ranges([lone_ref] * at + [ref], [lone_start] * at + [s], [1] * at + [hi - s + 1], [1] * (at + 1))
    # the slices: one row per leading range (its end lies outside the range: a work item that keeps nothing), then the run
    assert jx.expected(jr, rg)[0][at] == 0
    for ss, flt, anchor in itertools.product((False, True), FILTERS, (0, 8)):
        want = jx.expected(jr, rg, ss=ss, min_anchor=anchor, **flt)
        assert jx.same(query(reads, rg, ss=ss, min_anchor=anchor, **flt), want), (ss, flt, anchor)
    got = query(reads, rg)
    assert (got[1][0], got[2][0], got[3][0]) == (s, first_end, run_len)


def test_runs_filtered_in_the_middle_and_entirely(ctx):
    """hand-made: 300 reads across one junction whose middle 260 have mapq 0; three junctions A < B < C where every read of B
    carries 0x400"""
    reads = []
    for i in range(300):
        reads.append((0, 1000, 16 if i % 7 == 0 else 0, 0 if 20 <= i < 280 else 60, 0, "50M400N50M"))
    for k, (pos, flag) in enumerate(((5000, 0), (6000, 0x400), (7000, 0))):
        reads += [(0, pos, flag | (16 if j % 3 == 0 else 0), 60, 0, "30M200N70M") for j in range(70 + k)]
    cols = sx.columns([100_000], reads)
    jr = jx.rows(cols)
    r = upload(ctx, cols)
    assert r.n_junction_rows == len(jr["start"]) == 300 + 70 + 71 + 72
    rg = ranges([0, 0], [0, 900], [100_000, 7000], [1, -1])
    for ss, flt in itertools.product((False, True), (dict(), dict(mapqual=30), dict(filteredF=0x400), dict(mapqual=30, filteredF=0x400))):
        assert jx.same(query(r, rg, ss=ss, **flt), jx.expected(jr, rg, ss=ss, **flt)), (ss, flt)
    got = query(r, rg, mapqual=30)
    assert got[1].tolist()[:4] == [1050, 5030, 6030, 7030] and got[3].tolist()[:4] == [40, 70, 71, 72]
    got = query(r, rg, filteredF=0x400)
    assert got[0].tolist() == [0, 3, 6] and got[1].tolist()[:3] == [1050, 5030, 7030] and got[3].tolist()[:3] == [300, 70, 72]
    r.close()


# ---- identity with the shipped kernels --------------------------------------------------------------------------------------
def test_plain_minus_spliced_coverage_is_the_junctions(ctx, decks):
    cols, jr, reads = decks["junction"]
    rg = whole_references(cols)
    plain = upload(ctx, cols, spliced=False)
    prm = make_params(_lib.MODE_COVERAGE)
    cov = []
    for r in (plain, reads):
        plan = Plan(ctx, r, rg["rid"], rg["loc"], rg["len"], rg["strand"], prm)
        cov.append(plan.run_host().astype(np.int64))
        off = np.asarray(plan.offsets).copy()
        plan.close()
    seg_off, start, end, count, _ = query(reads, rg)
    want = np.zeros(len(cov[0]) + 1, dtype=np.int64)
    for i in range(len(rg["rid"])):
        a, b = seg_off[i], seg_off[i + 1]
        np.add.at(want, off[i] + start[a:b], count[a:b].astype(np.int64))
        np.add.at(want, off[i] + end[a:b] + 1, -count[a:b].astype(np.int64))
    assert np.array_equal(cov[0] - cov[1], np.cumsum(want)[:-1]) and count.sum() == len(jr["start"])
    plain.close()


# ---- file level -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deck_bam(tmp_path_factory):
    cols = jx.junction_deck()
    path = str(tmp_path_factory.mktemp("junctions") / "deck.bam")
    names = ["chr1", "chr2", "chr3"]
    write_columns_as_bam(path, names, {k: np.array(v) for k, v in cols.items()})
    return path, names, cols


def native(j):
    """a Junctions (1-based) as the handle-level tuple (0-based)"""
    return j.seg_off, j.start - 1, j.end - 1, j.count, j.max_anchor


@pytest.mark.parametrize("decode", ["all", "regions"])
def test_file_level(decks, deck_bam, monkeypatch, decode):
    path, names, cols = deck_bam
    _, jr, reads = decks["junction"]
    monkeypatch.setenv("BAMSIGNALS_DECODE", decode)
    lib = _lib.load()
    lib.bsig_cache_clear()
    g = jx.junction_genes()
    pick = np.r_[0:6, 10:16]                                # 12 genes, both references
    rg12 = {k: v[pick] for k, v in g.items()}
    gr12 = GRanges([names[r] for r in rg12["rid"]], rg12["loc"] + 1, width=rg12["len"], strand=["-*+"[s + 1] for s in rg12["strand"]])
    tiles = tile_ranges(cols["ref_len"], 5000)
    gr_cov = GRanges([names[r] for r in tiles["rid"]], tiles["loc"] + 1, width=tiles["len"])
    before = bamCoverage(path, gr_cov, verbose=False, splice=True)
    assert not last_call_timing()["bam_was_resident"] and "spliced" in last_call_route()
    whole = whole_references(cols)
    for ss, kw, flt in ((False, dict(), dict()), (True, dict(mapqual=30, filteredFlag=0x400, minAnchor=8), dict(mapqual=30, filteredF=0x400, min_anchor=8))):
        got = bamJunctions(path, ss=ss, verbose=False, **kw)
        route = last_call_route()
        assert "junctions" in route and "spliced" in route
        if decode == "all":
            assert last_call_timing()["bam_was_resident"] and "spliced, resident" in route, "the coverage call's spliced set"
        assert len(got) == 3 and jx.same(native(got), jx.expected(jr, whole, ss=ss, **flt))
        assert jx.same(native(got), query(reads, whole, ss=ss, **flt))
        got = bamJunctions(path, gr12, ss=ss, verbose=False, **kw)
        assert len(got) == 12 and got.njunctions > 0 and jx.same(native(got), jx.expected(jr, rg12, ss=ss, **flt))
        assert jx.same(native(got), query(reads, rg12, ss=ss, **flt))
        again = bamJunctions(path, gr12, ss=ss, verbose=False, **kw)
        assert last_call_timing()["bam_was_resident"] and "resident" in last_call_route() and "junctions" in last_call_route()
        assert jx.same(native(again), native(got))
        for a in (got.seg_off, got.start, got.end, got.count, got.max_anchor):
            assert not a.flags.writeable
    after = bamCoverage(path, gr_cov, verbose=False, splice=True)
    assert last_call_timing()["bam_was_resident"] and "spliced, resident" in last_call_route()
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(before, after))
    lib.bsig_cache_clear()
