"""GPU: bamOverlaps (modes BSIG_MODE_OVERLAP_ANY / _WITHIN, k_overlap / k_overlap_multi) against the numpy restatement
of its definition (tests/overlaps_expected.py: `restated`, which tests/test_overlaps_cpu.py holds against the C oracle),
exactly: a grid of widths on both sides of the 16,384-base tile, single reads planted on every seam (the anchor rule:
a read that overlaps several tiles counts once), the span classes' reach-back, heavy tiles and a pile past 16 bits, the
layouts, every kernel form by its launch-log name, template lengths of megabases, the plan's refusals and the file level."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

import forms_deck as deck
import overlaps_expected as oe
from test_overlaps_cpu import PARAM_RULE, overlap_params

pytestmark = pytest.mark.gpu

BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [2_000_000, 700_017]
STEP = 16384
PAIRED = {"ignore": dict(), "filter": dict(requiredF=66, tlen_filter=(0, 1000)),
          "extend": dict(requiredF=66, tlen_filter=(0, 1000), tspan=True)}


def _upload(ctx, cols):
    from bamsignals_amd.device import Reads
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])


@pytest.fixture(scope="module")
def synth():
    """paired reads on two references, resident on GPU 0 (the one upload the module shares)"""
    from bamsignals_amd.device import Context
    from bamsignals_amd.synth import synth_reads
    ctx = Context(0)
    cols = synth_reads(400_000, REF_LEN, seed=92, paired=True, with_cigar=False)
    reads = _upload(ctx, cols)
    yield ctx, cols, reads
    reads.close()
    ctx.close()


def _params(within=False, m=1, **kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    return make_params(_lib.MODE_OVERLAP_WITHIN if within else _lib.MODE_OVERLAP_ANY, binsize=m, **kw)


def _run(ctx, reads, rg, within=False, m=1, runs=2, **kw):
    """a plan's first run (fused lookups) and its second (windows kept), which must agree; (result, stats)"""
    from bamsignals_amd.device import Plan
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(within, m, **kw))
    try:
        n = len(rg["len"])
        assert plan.cells == n * (2 if kw.get("ss") else 1)
        got = [plan.run_host().copy() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        assert got[0].dtype == np.int32
        return got[0], plan.stats()
    finally:
        plan.close()


def _definition_kw(kw):
    return {k: v for k, v in kw.items() if k in ("ss", "tlen_filter", "mapqual", "requiredF", "filteredF", "tspan")}


def _check(ctx, reads, cols, rg, within=False, m=1, runs=2, **kw):
    got, st = _run(ctx, reads, rg, within, m, runs=runs, **kw)
    want = oe.restated(cols, rg, within=within, m=m, **_definition_kw(kw))
    assert np.array_equal(got, want), (within, m, kw, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    return got, st


def _ranges(n, w, seed):
    from bamsignals_amd.synth import synth_ranges
    return synth_ranges(n, w, REF_LEN, seed=seed)


def _cat(*rgs):
    return {k: np.concatenate([np.asarray(r[k], np.int32) for r in rgs]) for k in ("rid", "loc", "len", "strand")}


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 100, 16384, 16385, 40000])
def test_grid(synth, w):
    ctx, cols, reads = synth
    rg = _ranges(12 if w == 40000 else 60, w, seed=1000 + w)
    assert set(rg["strand"].tolist()) == {1, -1, 0}
    totals = {}
    for pe, kw in PAIRED.items():
        for within in (False, True):
            for m in (1, 30, 101):
                for ss in (False, True):
                    got, st = _check(ctx, reads, cols, rg, within, m, ss=ss, **kw)
                    assert st["n_items"] == len(rg["len"]) * ((w + STEP - 1) // STEP)
                    totals[pe, within, m, ss] = int(got.sum())
                assert totals[pe, within, m, False] == totals[pe, within, m, True]
    if w >= 100:
        for pe in PAIRED:
            assert totals[pe, False, 1, False] > totals[pe, False, 30, False] > 0
            # (a 100-base read is never inside a 100-base range with 101 bases of it)
            assert totals[pe, False, 1, False] > totals[pe, True, 1, False] > (0 if w > 100 else -1)
        assert totals["extend", False, 1, False] > totals["filter", False, 1, False]
    else:
        assert totals["ignore", False, 1, False] > 0 and totals["ignore", False, 30, False] == 0


def test_stats_are_a_count_plans(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, cols, reads = synth
    rg = _cat(_ranges(40, 300, seed=5), _ranges(6, 40000, seed=6))
    for kw, per_packed in ((dict(), 4), (dict(requiredF=66, tlen_filter=(0, 1000)), 8)):
        _, st = _run(ctx, reads, rg, runs=1, **kw)
        plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COUNT, binsize=-1, **kw))
        try:
            plan.run_host()
            want = plan.stats()
        finally:
            plan.close()
        assert st == want and st["visits_packed"] > 0 and st["bytes_per_visit_packed"] == per_packed
    _, st = _run(ctx, reads, rg, runs=1, **PAIRED["extend"])
    assert st["bytes_per_visit_packed"] == 8 and st["visits"] > want["visits"]       # (the windows reach out by tlen_filter[1])


# ---- seams -----------------------------------------------------------------------------------------------------------
def _seam_reads(lo, w, step, m, tf1):
    """single first mates (flag 99 forward / 83 reverse, 30 bases, tlen 0 unless said: the read is its own interval under
    every rule) on the range's ends and its tiles' seams, and fragments that reach the range from outside it"""
    hi, R = lo + w, 30
    parts = []

    def both(pos, span=R, tlen=0):
        parts.append(oe.planted(pos, span, flag=99, tlen=tlen))
        parts.append(oe.planted(pos, span, flag=83, tlen=tlen))
    for end in (lo - 1, lo):                                         # ending on lo - 1 / lo
        both(end - R + 1)
    for start in (hi - 1, hi):                                       # starting on hi - 1 / hi
        both(start)
    for x in range(lo + step, hi, step):                             # every seam, by one base either way
        for pos in (x - R, x - R + 1, x - 1, x):
            both(pos)
    both(lo - 50, w + 100)                                           # longer than the range, out on both sides
    for pos, span in ((lo, w), (lo - 1, w), (lo + 1, w), (lo - 1, w + 1), (lo, w + 1), (lo - 1, w + 2)):
        both(pos, span)                                              # within: an exact fit, one base over at either end
    for k in (m - 1, m, m + 1):                                      # k bases of overlap at either end
        both(lo + k - R)
        both(hi - k)
    # fragments (paired.end = "extend"): a forward first mate wholly left of the range, its fragment's last base on
    # lo - 11, lo, lo + 29, ... and past several seams; the other tlen sign does not extend; tf1 + 1 is filtered out
    for L in (190, 201, 230, 2 * step + 250 if 2 * step + 250 <= tf1 else tf1 - 1, tf1, tf1 + 1):
        parts.append(oe.planted(lo - 200, R, flag=99, tlen=L))
        parts.append(oe.planted(lo - 200, R, flag=99, tlen=-L))
        # ... and a reverse one whose read lies right of hi (its last base hi + 179), its fragment's first base on hi,
        # hi - 1, hi - 70, ...
    for L in (180, 181, 250, 2 * step + 250 if 2 * step + 250 <= tf1 else tf1 - 1, tf1, tf1 + 1):
        parts.append(oe.planted(hi + 150, R, flag=83, tlen=-L))
        parts.append(oe.planted(hi + 150, R, flag=83, tlen=L))
    # a reverse fragment inside the range whose first base lies in an earlier tile than its read (and its mirror image)
    parts.append(oe.planted(lo + 2 * step + 20, R, flag=83, tlen=-(step + 40)))
    parts.append(oe.planted(lo + 5, R, flag=99, tlen=2 * step + 30))
    return parts


@pytest.mark.parametrize("tile,w", [(64, 64 * 3 + 17), (0, 16384 * 2 + 100)])
def test_seams(synth, tile, w):
    """the test that catches double counting: a read that overlaps several tiles of its range counts in the tile of its
    anchor alone"""
    ctx = synth[0]
    lo, m = 40_000, 10
    step = tile or STEP
    tf1 = 2 * step + 1000
    cols = oe.merge_sorted(_seam_reads(lo, w, step, m, tf1), 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=[0, 0], loc=[lo, lo], len=[w, w], strand=[1, -1])
        rules = dict(read=dict(), extend=dict(requiredF=66, tlen_filter=(0, tf1), tspan=True))
        want = {(r, wi, mm): oe.restated(cols, rg, within=wi, m=mm, ss=True, **kw)
                for r, kw in rules.items() for wi in (False, True) for mm in (1, m)}
        # the planting took: reads on both strands and both sides of every threshold
        n_seams = (w - 1) // step
        # (per strand: one of the two reads at either end of the range, four a seam, the long one, the six around an
        # exact fit, three overlaps at either end, one read of the last two fragments; 1 base of overlap at either end
        # and m - 1 at either end fall to minoverlap m; inside are at most the seams' reads, the exact fit and that last read;
        # four fragments a side reach in from outside)
        per_strand = 2 + 4 * n_seams + 1 + 6 + 6 + 1
        assert want["read", False, 1][:2].tolist() == [per_strand, per_strand]
        assert want["read", False, m][:2].tolist() == [per_strand - 4, per_strand - 4]
        assert 2 <= want["read", True, 1][0] <= 4 * n_seams + 2 and want["read", True, 1][0] == want["read", True, 1][1]
        assert want["extend", False, 1][:2].tolist() == [per_strand + 4, per_strand + 4]
        assert np.array_equal(want["read", False, 1][2:], want["read", False, 1][1::-1])      # the '-' range swaps the rows
        for (r, wi, mm), expect in want.items():
            for threads in (64, 256):
                got, st = _run(ctx, reads, rg, wi, mm, ss=True, tile_cells=tile, threads=threads, **rules[r])
                assert np.array_equal(got, expect), (r, wi, mm, threads, got, expect)
                assert st["n_items"] == 2 * ((w + step - 1) // step)
    finally:
        reads.close()


# ---- span classes ----------------------------------------------------------------------------------------------------
def test_span_classes_reach_back(synth):
    """ranges just inside a long read's far end see it through its class's reach-back (maxspan), ranges just behind the
    end do not; one range of 300,000 bases under a 200,000-base read: 19 tiles, the read counted once"""
    ctx = synth[0]
    rng = np.random.default_rng(17)
    ref = 1_000_000
    n_bg = 4000
    bg = rng.integers(0, ref - 100, n_bg)
    parts = [dict(rid=np.zeros(n_bg, np.int64), pos=bg, end=bg + rng.integers(20, 101, n_bg) - 1,
                  flag=np.where(rng.random(n_bg) < 0.5, 16, 0), mapq=np.full(n_bg, 40), tlen=np.zeros(n_bg, np.int64))]
    long_reads = []
    for span, starts in ((3_000, (50_000, 300_000, 650_000)), (50_000, (120_000, 400_000, 700_000)), (200_000, (350_000, 610_000))):
        for k, p in enumerate(starts):
            parts.append(oe.planted(p, span, reverse=bool(k & 1)))
            long_reads.append((p, span))
    cols = oe.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([ref], np.int64)
    reads = _upload(ctx, cols)
    try:
        info = reads.info()
        assert all(info["class_n"][c] > 0 for c in (1, 2, 3))
        loc, w = [], []
        for p, span in long_reads:
            e = p + span - 1
            loc += [e - 99, e - 120, e + 1, e, p - 100, p - 99]
            w += [100] * 6
        loc.append(350_000 - 50_000)
        w.append(300_000)
        rg = dict(rid=np.zeros(len(loc), np.int32), loc=np.asarray(loc, np.int32), len=np.asarray(w, np.int32),
                  strand=np.resize([1, -1, 0], len(loc)).astype(np.int32))
        for within in (False, True):
            for m in (1, 50):
                for ss in (False, True):
                    got, st = _check(ctx, reads, cols, rg, within, m, ss=ss)
        assert st["n_items"] == len(loc) - 1 + 19
        # the long read is there in the ranges inside its end, and gone one base behind it
        bg_only = oe.restated(dict(cols, **{k: cols[k][cols["end"] - cols["pos"] < 200] for k in ("pos", "end", "flag", "mapq", "tlen")},
                                   ref_off=np.asarray([0, n_bg], np.int64)), rg)
        full = oe.restated(cols, rg)
        d = (full - bg_only)[:-1].reshape(-1, 6)          # long reads per range (some lie under another long read)
        assert np.all(d[:, 0] >= 1) and np.all(d[:, 1] == d[:, 0]) and np.all(d[:, 3] == d[:, 0]) and np.all(d[:, 5] >= 1)
        assert np.all(d[:, 2] == d[:, 0] - 1) and np.all(d[:, 4] == d[:, 5] - 1)
        assert full[-1] - bg_only[-1] >= 3
    finally:
        reads.close()


# ---- heavy tiles -----------------------------------------------------------------------------------------------------
def test_heavy_tiles_are_sliced(synth, monkeypatch):
    ctx, cols, reads = synth
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    rg = _cat(_ranges(30, 16385, seed=31), _ranges(30, 100, seed=32))
    for pe in ("ignore", "extend"):
        for within, m, ss in ((False, 1, True), (True, 30, False)):
            got, st = _check(ctx, reads, cols, rg, within, m, ss=ss, **PAIRED[pe])
            assert st["heavy_tiles"] >= 30 and got.sum() > 0


def test_pile_on_one_base(synth):
    """70,000 reads over one base: past the 16-bit halves of the packed counter and the 32,768-read ceiling of a tile"""
    ctx = synth[0]
    at, n = 50_000, 70_000
    rng = np.random.default_rng(3)
    parts = [dict(rid=np.zeros(n, np.int64), pos=np.full(n, at - 20), end=np.full(n, at + 19),
                  flag=np.where(np.arange(n) < 41_000, 0, 16), mapq=np.full(n, 30), tlen=np.zeros(n, np.int64))]
    p = rng.integers(45_000, 56_000, 3000)
    parts.append(dict(rid=np.zeros(3000, np.int64), pos=p, end=p + 49, flag=np.where(rng.random(3000) < 0.5, 0, 16),
                      mapq=np.full(3000, 30), tlen=np.zeros(3000, np.int64)))
    cols = oe.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([200_000], np.int64)
    reads = _upload(ctx, cols)
    try:
        rg = dict(rid=np.zeros(6, np.int32), loc=np.asarray([49_000, 49_000, 49_000, at, at - 20, at + 20], np.int32),
                  len=np.asarray([3000, 3000, 3000, 1, 40, 100], np.int32), strand=np.asarray([1, -1, 0, 1, -1, 1], np.int32))
        for within in (False, True):
            got, st = _check(ctx, reads, cols, rg, within, 1, ss=True)
            assert st["heavy_tiles"] >= 5
            assert got[0] >= 41_000 > 2 ** 15 and got[1] >= 29_000 and got[2] == got[1] and got[3] == got[0]
        assert got[2 * 4] == 29_000 and got[2 * 4 + 1] == 41_000 and got[2 * 3] == 0      # within: the exact fit; none in one base
        got, _ = _check(ctx, reads, cols, rg, False, 1, ss=False)
        assert got[0] >= 70_000 > 2 ** 16
    finally:
        reads.close()


# ---- layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"BAMSIGNALS_PACK": "0"}, {"BAMSIGNALS_PACKED_HALF": "0"}])
def test_layouts(synth, env, monkeypatch):
    ctx, cols, _ = synth
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads = _upload(ctx, cols)
    try:
        rg = _cat(_ranges(40, 2500, seed=11), _ranges(4, 40000, seed=12))
        for pe, kw in PAIRED.items():
            for within, m in ((False, 1), (True, 1), (False, 101)):
                got, st = _check(ctx, reads, cols, rg, within, m, ss=True, **kw)
                assert got.sum() > 0
                assert (st["visits_packed"] > 0) == (env.get("BAMSIGNALS_PACK") != "0")
                # the diagnostic knob (read when a plan is made): packed reads through the per-read body, same counts
                monkeypatch.setenv("BAMSIGNALS_OVERLAP_QUAD", "0")
                wide, _ = _run(ctx, reads, rg, within, m, runs=1, ss=True, **kw)
                monkeypatch.delenv("BAMSIGNALS_OVERLAP_QUAD")
                assert np.array_equal(wide, got), (pe, within, m)
    finally:
        reads.close()


# ---- the kernel forms ------------------------------------------------------------------------------------------------
OVERLAP_FORMS = tuple(f"k_overlap<{nt},within={wi}> acc={acc}" for nt in (64, 128, 256) for wi in (0, 1) for acc in (0, 1)) + \
                tuple(f"k_overlap_multi<T={t},pre={pre},within={wi}> acc=0" for t in (4, 8) for pre in (2, 4) for wi in (0, 1))
SEEN = set()
# the deck's parameter sets: the packed class's own body (no template-length rule), and the per-read body under one
DECK_SETS = {"plain": dict(mapqual=10, ss=True), "extend": dict(tlen_filter=(0, 400), tspan=True, ss=True)}
DECK_M = 5


@pytest.fixture(scope="module")
def deck_gpu():
    from bamsignals_amd.device import Context, Reads
    c = deck.reads()
    ctx = Context(0)
    out = {}
    old = os.environ.get("BAMSIGNALS_PACK")
    try:
        for layout in ("packed", "nopack"):
            if layout == "nopack":
                os.environ["BAMSIGNALS_PACK"] = "0"
            out[layout] = Reads(ctx, c["ref_len"], c["ref_off"], c["pos"], c["flag"], c["mapq"], c["tlen"], end=c["end"])
    finally:
        if old is None:
            os.environ.pop("BAMSIGNALS_PACK", None)
        else:
            os.environ["BAMSIGNALS_PACK"] = old
    yield ctx, out
    for r in out.values():
        r.close()
    ctx.close()


@functools.lru_cache(maxsize=None)
def _deck_expected(pset, within):
    want = oe.restated(deck.reads(), deck.ranges(), within=within, m=DECK_M, **DECK_SETS[pset])
    want.setflags(write=False)
    return want


def _deck_case(deck_gpu, layout, pset, within, expect, knobs, threads=0, heavy=False):
    """test_kernel_forms_gpu.py's case for an overlap plan: knobs set, log on, two runs against the definition, the log
    against `expect`"""
    from test_kernel_forms_gpu import _selected
    from bamsignals_amd.device import Plan
    ctx, reads = deck_gpu
    rg, want = deck.ranges(), _deck_expected(pset, within)
    with _selected(knobs, heavy=heavy) as drain:
        plan = Plan(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(within, DECK_M, threads=threads, **DECK_SETS[pset]))
        try:
            first, second, st = plan.run_host().copy(), plan.run_host().copy(), plan.stats()
        finally:
            plan.close()
        names = drain()
    SEEN.update(names)
    assert want.sum() > 10_000
    assert np.array_equal(first, want), (names, int(np.sum(first != want)))
    assert np.array_equal(second, want), (names, int(np.sum(second != want)))       # (the resolved form: windows kept)
    assert set(names) == set(expect) and len(names) == (4 if heavy else 2), (names, expect)
    assert (st["heavy_tiles"] > 0) == heavy


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("within", [False, True])
@pytest.mark.parametrize("nt", [64, 128, 256])
@pytest.mark.parametrize("layout,pset", [("packed", "plain"), ("packed", "extend"), ("nopack", "plain")])
def test_forms_one_tile_per_workgroup(deck_gpu, layout, pset, nt, within, heavy):
    form = f"k_overlap<{nt},within={int(within)}> acc=%d"
    _deck_case(deck_gpu, layout, pset, within, [form % 0] + ([form % 1] if heavy else []), {1: 1}, threads=nt, heavy=heavy)


@pytest.mark.parametrize("within", [False, True])
@pytest.mark.parametrize("pre", [2, 4])
@pytest.mark.parametrize("per_wave", [4, 8])
@pytest.mark.parametrize("layout,pset", [("packed", "plain"), ("packed", "extend"), ("nopack", "plain")])
def test_forms_several_tiles_per_wave(deck_gpu, layout, pset, per_wave, pre, within):
    _deck_case(deck_gpu, layout, pset, within, [f"k_overlap_multi<T={per_wave},pre={pre},within={int(within)}> acc=0"],
               {1: per_wave, 2: pre}, threads=64)


def test_forms_seen_are_the_list_and_a_count_plan_launches_none(deck_gpu):
    """runs after the cases above (pytest keeps a module's order)"""
    from test_kernel_forms_gpu import _selected
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    assert len(set(OVERLAP_FORMS)) == len(OVERLAP_FORMS) == 20
    assert SEEN == set(OVERLAP_FORMS), dict(never_reached=sorted(set(OVERLAP_FORMS) - SEEN), not_listed=sorted(SEEN - set(OVERLAP_FORMS)))
    ctx, reads = deck_gpu
    rg = deck.ranges()
    with _selected({}, heavy=True) as drain:
        plans = [Plan(ctx, reads["packed"], rg["rid"], rg["loc"], rg["len"], rg["strand"], p)
                 for p in (make_params(_lib.MODE_COUNT, binsize=-1, ss=True), _params(False, DECK_M, ss=True))]
        try:
            count = plans[0].run_host().copy()
            names_count = drain()
            plans[1].run_host()
            names_overlap = drain()
            assert np.array_equal(plans[0].run_host(), count)
            names_count += drain()
        finally:
            for p in plans:
                p.close()
    assert names_count and all(n.startswith("k_count") for n in names_count), names_count
    assert names_overlap and all(n.startswith("k_overlap") for n in names_overlap), names_overlap
    assert np.array_equal(count, deck.expected("count")[0])


# ---- megabases -------------------------------------------------------------------------------------------------------
def test_megabase_fragments(synth):
    """fragments of megabases under "extend": the reach of the windows, and no 24-bit arithmetic on a length"""
    ctx = synth[0]
    ref = 64_000_000
    tf = (0, 20_000_000)
    big = [4_194_303, 4_194_304, 5_000_001, 19_999_999]
    parts, far = [], []
    for k, L in enumerate(big):
        p = 1_000_000 + 3_000_017 * k
        parts.append(oe.planted(np.full(1 + k, p), 40, flag=99, tlen=L))                   # forward: last base p + L - 1
        q = p + L - 1 + 5000                                                                # reverse: its read ends on q,
        parts.append(oe.planted(np.full(2, q - 39), 40, flag=83, tlen=-L))                  # first base q - L + 1
        far += [p + L - 1, q - L + 1]
    rng = np.random.default_rng(7)
    n_bg = 3000
    bg_pos = rng.integers(0, ref - 25_000_000, n_bg)
    parts.append(dict(rid=np.zeros(n_bg, np.int64), pos=bg_pos, end=bg_pos + 49, flag=np.where(rng.random(n_bg) < 0.5, 99, 163),
                      mapq=np.full(n_bg, 40), tlen=rng.integers(50, 21_000_000, n_bg)))
    cols = oe.merge_sorted(parts, 1)
    cols["ref_len"] = np.asarray([ref], np.int64)
    reads = _upload(ctx, cols)
    try:
        far = np.asarray(far, np.int64)
        # around every fragment's far end, just past it (forward: behind the last base; reverse: before the first), and
        # one range of six megabases
        loc = np.concatenate([far - 700, far[0::2] + 1, far[1::2] - 1500, [20_000_000]])
        w = np.concatenate([np.full(len(far) + len(far), 1500), [6_000_000]])
        rg = dict(rid=np.zeros(len(loc), np.int32), loc=loc.astype(np.int32), len=w.astype(np.int32),
                  strand=np.resize([1, -1, 0], len(loc)).astype(np.int32))
        kw = dict(requiredF=66, tlen_filter=tf, tspan=True)
        want = oe.restated(cols, rg, **kw)
        plain = oe.restated(cols, rg, requiredF=66, tlen_filter=tf)
        for k in range(len(big)):
            assert want[2 * k] - plain[2 * k] >= 1 + k and want[2 * k + 1] - plain[2 * k + 1] >= 2
        assert want[-1] > plain[-1] + 50
        for within in (False, True):
            for m in (1, 800):
                for ss in (False, True):
                    _check(ctx, reads, cols, rg, within, m, runs=1 if ss else 2, ss=ss, **kw)
    finally:
        reads.close()


# ---- errors and plans ------------------------------------------------------------------------------------------------
def test_errors(synth):
    """the parameter rule's table (tests/test_overlaps_cpu.py) through Plan, and what else a plan refuses"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, HistPlan, Plan, SumPlan, make_params
    ctx, cols, reads = synth
    a = ([0], [10], [100], [1])
    for mode in (_lib.MODE_OVERLAP_ANY, _lib.MODE_OVERLAP_WITHIN):
        for kw, code, message in PARAM_RULE:
            with pytest.raises(_lib.BsigError) as e:
                Plan(ctx, reads, *a, overlap_params(mode, kw))
            assert (e.value.code, str(e.value)) == (code, message)
    with pytest.raises(_lib.BsigError) as e:
        Plan(ctx, reads, [5], [10], [100], [1], _params())
    assert e.value.code_name == "BSIG_ERR_CHROM"
    with pytest.raises(_lib.BsigError, match="negative width"):
        Plan(ctx, reads, [0], [10], [-1], [1], _params())
    with pytest.raises(_lib.BsigError, match="unknown mode 6"):
        Plan(ctx, reads, *a, make_params(6))
    # no reduction is built on an overlap plan
    with pytest.raises(_lib.BsigError, match="bamCount has no sum over ranges"):
        SumPlan(ctx, reads, *a, _params())
    with pytest.raises(_lib.BsigError, match="defined on bamCount"):
        FragPlan(ctx, reads, *a, _params(tlen_filter=(0, 100), requiredF=66), 1)
    with pytest.raises(_lib.BsigError, match="one cell per range"):
        HistPlan(ctx, reads, *a, _params(), 10)


def test_runs_are_refused_and_a_stale_plan_too(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan
    ctx, cols, _ = synth
    lib = _lib.load()
    reads = _upload(ctx, cols)
    try:
        rg = _ranges(20, 300, seed=77)
        plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(ss=True))
        with pytest.raises(_lib.BsigError, match="bamCount has no runs: one cell per range") as e:
            plan.runs()
        assert e.value.code_name == "BSIG_ERR_ARG"
        first = plan.run_host().copy()
        assert np.array_equal(first, oe.restated(cols, rg, ss=True)) and first.any()
        assert lib.bsig_debug_new_layout_gen(reads._h) == 0
        with pytest.raises(_lib.BsigError, match="make a new plan"):
            plan.run_host()
        again = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], _params(ss=True))
        assert np.array_equal(again.run_host(), first)
        plan.close()
        again.close()
    finally:
        reads.close()


def test_zero_width_and_empty(synth):
    ctx, cols, reads = synth
    rg = dict(rid=[0, 1, 0, 0], loc=[5000, 100, 5000, -50], len=[0, 0, 300, 0], strand=[1, -1, 0, 1])
    for ss in (False, True):
        got, _ = _check(ctx, reads, cols, rg, ss=ss)
        assert got.reshape(4, -1)[[0, 1, 3]].sum() == 0 and got.sum() > 0
    empty = dict(rid=[], loc=[], len=[], strand=[])
    got, st = _run(ctx, reads, empty)
    assert got.size == 0 and st["n_items"] == 0


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
    w[:3] = (0, 1, 2)
    loc = np.asarray([rng.integers(0, int(fx["ref_len"][r]) - 100) for r in rid], np.int32)
    strand = np.asarray([1, -1, 0], np.int32)[rng.integers(0, 3, n)]
    gr = GRanges([names[r] for r in rid], loc + 1, width=w, strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in strand])
    return gr, dict(rid=rid, loc=loc, len=w, strand=strand), oe.fixture_columns(fx), names


@pytest.fixture(params=["all", "regions"])
def decode_mode(request, monkeypatch):
    from bamsignals_amd import _lib
    monkeypatch.setenv("BAMSIGNALS_DECODE", request.param)
    _lib.load().bsig_cache_clear()
    yield request.param
    _lib.load().bsig_cache_clear()


def test_file_level(fixture, decode_mode):
    from bamsignals_amd import bamOverlaps
    gr, rg, cols, _ = fixture
    total = 0
    for pe, kw in PAIRED.items():
        for kind in ("any", "within"):
            for ss in (False, True):
                for m in (1, 25):
                    got = bamOverlaps(BAM, gr, type=kind, minoverlap=m, ss=ss, paired_end=pe, verbose=False)
                    want = oe.restated(cols, rg, within=kind == "within", m=m, ss=ss, **kw)
                    assert got.dtype == np.int32 and got.shape == ((2, len(gr)) if ss else (len(gr),))
                    assert np.array_equal(got.T.reshape(-1), want), (pe, kind, ss, m)
                    total += int(got.sum())
    assert total > 10_000
    got = bamOverlaps(BAM, gr, mapqual=30, filteredFlag=1024, paired_end="extend", tlenFilter=(50, 300), verbose=False)
    assert np.array_equal(got, oe.restated(cols, rg, mapqual=30, filteredF=1024, requiredF=66, tlen_filter=(50, 300), tspan=True))


def test_a_width_one_range_is_the_coverage_cell(fixture, decode_mode):
    """a product-level identity: the reads that overlap one base are the reads that cover it"""
    from bamsignals_amd import GRanges, bamCoverage, bamOverlaps
    names, cols = fixture[3], fixture[2]
    rng = np.random.default_rng(5)
    n = 300
    rid = rng.integers(0, len(names), n)
    start = np.asarray([rng.integers(1, int(cols["ref_len"][r])) for r in rid])
    gr = GRanges([names[r] for r in rid], start, width=np.ones(n, np.int32), strand=["*"] * n)
    for pe in ("ignore", "extend"):
        cov = bamCoverage(BAM, gr, paired_end=pe, verbose=False)
        cells = np.asarray([int(s[0]) for s in cov], np.int32)
        assert np.array_equal(bamOverlaps(BAM, gr, paired_end=pe, verbose=False), cells) and cells.sum() > 0


def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import _lib, bamOverlaps
    from bamsignals_amd.wrappers import last_call_route
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
        one = bamOverlaps(BAM, gr, ss=True, paired_end="extend", verbose=False)
        assert "1 GPU slot(s)" in last_call_route()
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
        four = bamOverlaps(BAM, gr, ss=True, paired_end="extend", verbose=False)
        assert "4 GPU slot(s)" in last_call_route()
        assert np.array_equal(one, four) and one.any()
    finally:
        _lib.load().bsig_cache_clear()
