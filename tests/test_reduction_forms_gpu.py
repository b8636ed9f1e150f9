"""GPU: every form of the five reductions' tile kernels that xcorr_form, frag_form, hist_form,
summary_form and scaled_form (csrc/kernels.hip) can launch -- 9 + 12 + 30 + 15 + 24 = 90 instantiations -- run
on tests/forms_deck.py's reads and ranges and compared with the C oracle's per-base cells reduced in numpy
(forms_deck.expected_xcorr / _frag / _hist / _summary / _scaled), exactly, in int64.  A case is
test_kernel_forms_gpu.py's: the call parameters and environment that select one form are set, the launch log is turned on
(bsig_debug_launch_log), the plan is made and run twice -- the first run looks its windows up in the kernel, the second
reads the kept ones --, and the log must hold exactly the forms the case names.  The last test holds the list of all 90
names and compares it with what the cases saw: a form nobody reached fails it, and so does a form nobody listed.

Three read sets: `packed`, the default layout, where span classes 0 and 1 are read from their 16-bit 5'-end columns
(bytes_per_visit_short 2) beside the packed class's (bytes_per_visit_packed 2); `packed_noshort`, made under
BAMSIGNALS_SHORT_HALF=0, where the half forms read classes 0 and 1 from pos + fm (8) and the packed class's column (2);
`nopack`, made under BAMSIGNALS_PACK=0, which has no packed class and runs the word forms only.  On the packed layouts a
word form is reached with mapqual=10, a filter that rejects some of the pair table's codes.  The deck's class-0 islands put
column windows of exactly NT - 1, NT, NT + 1 reads (one half-word per lane, or eight) and 8 NT - 1, 8 NT, 8 NT + 1 reads
(the eight-per-lane loop's trips) at every alignment in front of every workgroup size; its paired islands do the same for
the fragment-length histogram's packed-class body.

Wide forms (a 32-bit image, one tile per workgroup in a second launch) come from BAMSIGNALS_HEAVY_READS=64: such a case
logs its main form and its wide form.  BAMSIGNALS_FRAG_FORM, BAMSIGNALS_HIST_FORM and BAMSIGNALS_SCALED_SEGMENTED choose
among the consumers; all three are read when the plan is made.

The ranges are the deck's as they are -- widths 0 .. 9, duplicates, ranges hanging over both ends of a reference: no
kind refuses any of them."""
import contextlib
import os

import numpy as np
import pytest

import forms_deck as deck

pytestmark = pytest.mark.gpu

SEEN = set()            # every form name a case of this module logged (test_every_form_was_reached reads it)
NTS = (64, 128, 256)
LAYOUTS = {"packed": {}, "packed_noshort": {"BAMSIGNALS_SHORT_HALF": "0"}, "nopack": {"BAMSIGNALS_PACK": "0"}}
BYTES_PER_VISIT = {"packed": (2, 2), "packed_noshort": (8, 2)}       # (short, packed) of a half form

ALL_FORMS = (
    "k_xcorr_tiles<64,half=1,wide=0>",
    "k_xcorr_tiles<64,half=0,wide=0>",
    "k_xcorr_tiles<64,half=0,wide=1>",
    "k_xcorr_tiles<128,half=1,wide=0>",
    "k_xcorr_tiles<128,half=0,wide=0>",
    "k_xcorr_tiles<128,half=0,wide=1>",
    "k_xcorr_tiles<256,half=1,wide=0>",
    "k_xcorr_tiles<256,half=0,wide=0>",
    "k_xcorr_tiles<256,half=0,wide=1>",
    "k_frag_tiles<64,merge=0,ltab=1>",
    "k_frag_tiles<64,merge=0,ltab=0>",
    "k_frag_tiles<64,merge=1,ltab=1>",
    "k_frag_tiles<64,merge=1,ltab=0>",
    "k_frag_tiles<128,merge=0,ltab=1>",
    "k_frag_tiles<128,merge=0,ltab=0>",
    "k_frag_tiles<128,merge=1,ltab=1>",
    "k_frag_tiles<128,merge=1,ltab=0>",
    "k_frag_tiles<256,merge=0,ltab=1>",
    "k_frag_tiles<256,merge=0,ltab=0>",
    "k_frag_tiles<256,merge=1,ltab=1>",
    "k_frag_tiles<256,merge=1,ltab=0>",
    "k_hist_tiles<64,kHistCover,wide=0,form=0>",
    "k_hist_tiles<64,kHistCover,wide=1,form=0>",
    "k_hist_tiles<64,kHistEnds,wide=0,form=0>",
    "k_hist_tiles<64,kHistEnds,wide=1,form=0>",
    "k_hist_tiles<64,kHistEndsHalf,wide=0,form=0>",
    "k_hist_tiles<64,kHistCover,wide=0,form=1>",
    "k_hist_tiles<64,kHistCover,wide=1,form=1>",
    "k_hist_tiles<64,kHistEnds,wide=0,form=1>",
    "k_hist_tiles<64,kHistEnds,wide=1,form=1>",
    "k_hist_tiles<64,kHistEndsHalf,wide=0,form=1>",
    "k_hist_tiles<128,kHistCover,wide=0,form=0>",
    "k_hist_tiles<128,kHistCover,wide=1,form=0>",
    "k_hist_tiles<128,kHistEnds,wide=0,form=0>",
    "k_hist_tiles<128,kHistEnds,wide=1,form=0>",
    "k_hist_tiles<128,kHistEndsHalf,wide=0,form=0>",
    "k_hist_tiles<128,kHistCover,wide=0,form=1>",
    "k_hist_tiles<128,kHistCover,wide=1,form=1>",
    "k_hist_tiles<128,kHistEnds,wide=0,form=1>",
    "k_hist_tiles<128,kHistEnds,wide=1,form=1>",
    "k_hist_tiles<128,kHistEndsHalf,wide=0,form=1>",
    "k_hist_tiles<256,kHistCover,wide=0,form=0>",
    "k_hist_tiles<256,kHistCover,wide=1,form=0>",
    "k_hist_tiles<256,kHistEnds,wide=0,form=0>",
    "k_hist_tiles<256,kHistEnds,wide=1,form=0>",
    "k_hist_tiles<256,kHistEndsHalf,wide=0,form=0>",
    "k_hist_tiles<256,kHistCover,wide=0,form=1>",
    "k_hist_tiles<256,kHistCover,wide=1,form=1>",
    "k_hist_tiles<256,kHistEnds,wide=0,form=1>",
    "k_hist_tiles<256,kHistEnds,wide=1,form=1>",
    "k_hist_tiles<256,kHistEndsHalf,wide=0,form=1>",
    "k_summary_tiles<64,kHistCover,wide=0>",
    "k_summary_tiles<64,kHistCover,wide=1>",
    "k_summary_tiles<64,kHistEnds,wide=0>",
    "k_summary_tiles<64,kHistEnds,wide=1>",
    "k_summary_tiles<64,kHistEndsHalf,wide=0>",
    "k_summary_tiles<128,kHistCover,wide=0>",
    "k_summary_tiles<128,kHistCover,wide=1>",
    "k_summary_tiles<128,kHistEnds,wide=0>",
    "k_summary_tiles<128,kHistEnds,wide=1>",
    "k_summary_tiles<128,kHistEndsHalf,wide=0>",
    "k_summary_tiles<256,kHistCover,wide=0>",
    "k_summary_tiles<256,kHistCover,wide=1>",
    "k_summary_tiles<256,kHistEnds,wide=0>",
    "k_summary_tiles<256,kHistEnds,wide=1>",
    "k_summary_tiles<256,kHistEndsHalf,wide=0>",
    "k_scaled_tiles<64,kHistCover,wide=0,seg=0>",
    "k_scaled_tiles<64,kHistCover,wide=0,seg=1>",
    "k_scaled_tiles<64,kHistCover,wide=1,seg=0>",
    "k_scaled_tiles<64,kHistEnds,wide=0,seg=0>",
    "k_scaled_tiles<64,kHistEnds,wide=0,seg=1>",
    "k_scaled_tiles<64,kHistEnds,wide=1,seg=0>",
    "k_scaled_tiles<64,kHistEndsHalf,wide=0,seg=0>",
    "k_scaled_tiles<64,kHistEndsHalf,wide=0,seg=1>",
    "k_scaled_tiles<128,kHistCover,wide=0,seg=0>",
    "k_scaled_tiles<128,kHistCover,wide=0,seg=1>",
    "k_scaled_tiles<128,kHistCover,wide=1,seg=0>",
    "k_scaled_tiles<128,kHistEnds,wide=0,seg=0>",
    "k_scaled_tiles<128,kHistEnds,wide=0,seg=1>",
    "k_scaled_tiles<128,kHistEnds,wide=1,seg=0>",
    "k_scaled_tiles<128,kHistEndsHalf,wide=0,seg=0>",
    "k_scaled_tiles<128,kHistEndsHalf,wide=0,seg=1>",
    "k_scaled_tiles<256,kHistCover,wide=0,seg=0>",
    "k_scaled_tiles<256,kHistCover,wide=0,seg=1>",
    "k_scaled_tiles<256,kHistCover,wide=1,seg=0>",
    "k_scaled_tiles<256,kHistEnds,wide=0,seg=0>",
    "k_scaled_tiles<256,kHistEnds,wide=0,seg=1>",
    "k_scaled_tiles<256,kHistEnds,wide=1,seg=0>",
    "k_scaled_tiles<256,kHistEndsHalf,wide=0,seg=0>",
    "k_scaled_tiles<256,kHistEndsHalf,wide=0,seg=1>",
)


# ---------------------------------------------------------------------------------------------------------------
# the reads in three layouts, the environment, one case
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(values):
    """environment variables set (None: unset) and put back"""
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def gpu():
    """(context, {layout: Reads}): the deck's reads in the three layouts"""
    from bamsignals_amd.device import Context, Reads
    c = deck.reads()
    ctx = Context(0)
    out = {}
    for layout, env in LAYOUTS.items():
        with _env({"BAMSIGNALS_SHORT_HALF": None, "BAMSIGNALS_PACK": None, "BAMSIGNALS_PACKED_HALF": None, **env}):
            out[layout] = Reads(ctx, c["ref_len"], c["ref_off"], c["pos"], c["flag"], c["mapq"], c["tlen"], end=c["end"])
    info = {k: r.info() for k, r in out.items()}
    cls = np.bincount(deck.read_classes(True), minlength=5)
    for layout in ("packed", "packed_noshort"):
        assert list(info[layout]["class_n"][:5]) == cls.tolist(), layout      # class 0: the bulk's 1,098 and the class-0 islands
    assert info["nopack"]["class_n"][4] == 0
    yield ctx, out
    for r in out.values():
        r.close()
    ctx.close()


def _params(signal, ss=False, **kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    if signal == "coverage":
        return make_params(_lib.MODE_COVERAGE, **kw)
    if signal == "frag":
        return make_params(_lib.MODE_COUNT, binsize=-1, requiredF=66, **kw)
    return make_params(_lib.MODE_PROFILE, binsize=1, ss=ss, **kw)


def _case(gpu, layout, make, want, expect, env=None, heavy=False, half=False):
    """One case: make(ctx, reads, range arrays) -> the plan, made with `env` set; both runs against `want`, the log against
    `expect`, heavy tiles iff asked for, and for a half form the bytes a visit of classes 0 / 1 and of the packed class reads."""
    from test_kernel_forms_gpu import _selected
    ctx, reads = gpu
    rg = deck.ranges()
    with _selected({}, heavy=heavy) as drain, _env(env or {}):
        plan = make(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"])
        try:
            first, second, st = plan.run_host().copy(), plan.run_host().copy(), plan.stats()
        finally:
            plan.close()
        names = drain()
    SEEN.update(names)
    want = np.asarray(want)
    assert want.any() and want.dtype == np.int64 and first.dtype == np.int64
    assert first.shape == want.shape, (first.shape, want.shape)
    assert np.array_equal(first, want), (names, int(np.sum(first != want)), np.argwhere(first != want)[:8].tolist())
    assert np.array_equal(second, want), (names, int(np.sum(second != want)), np.argwhere(second != want)[:8].tolist())
    assert set(names) == set(expect), (names, expect)
    assert (st["heavy_tiles"] > 0) == heavy
    if half:
        assert (st["bytes_per_visit_short"], st["bytes_per_visit_packed"]) == BYTES_PER_VISIT[layout], layout
        assert st["visits_short"] > 0
    return st


def _reads_kind(layout, word):
    """(is it a half form, the filter that makes it the word form on a packed layout)"""
    half = layout != "nopack" and not word
    return half, (10 if word and layout != "nopack" else 0)


# ---------------------------------------------------------------------------------------------------------------
# strand cross-correlation: k_xcorr_tiles<NT, half, wide>
# ---------------------------------------------------------------------------------------------------------------
# (layout, word form, max_lag, body cells, heavy).  max_lag 0, 31 and 32: both sides of 2 * (max_lag + 1) <= NT for NT 64;
# 0 / 31 and 32 / 200: the two-lags-per-pass loop without and with a second lag; 2,047: the largest LDS shape.  Every lag
# and both bodies meet the 16-bit columns of the default layout at every NT.
XCORR = [("packed", False, 0, 16, False), ("packed", False, 31, 2048, False), ("packed", False, 32, 16, False),
         ("packed", False, 200, 2048, False), ("packed", False, 2047, 16, False), ("packed", False, 2047, 2048, False),
         ("packed_noshort", False, 31, 16, False), ("packed_noshort", False, 200, 2048, False),
         ("packed", True, 200, 2048, False), ("nopack", False, 32, 16, False), ("nopack", False, 2047, 2048, False),
         ("packed", False, 200, 2048, True), ("nopack", False, 31, 16, True)]


@pytest.mark.parametrize("layout,word,max_lag,body,heavy", XCORR)
@pytest.mark.parametrize("nt", NTS)
def test_xcorr(gpu, nt, layout, word, max_lag, body, heavy):
    from bamsignals_amd.device import XcorrPlan
    half, mapqual = _reads_kind(layout, word)
    form = f"k_xcorr_tiles<{nt},half=%d,wide=%d>"
    _case(gpu, layout, lambda *a: XcorrPlan(*a, _params("ends", mapqual=mapqual, tile_cells=body, threads=nt), max_lag),
          deck.expected_xcorr(max_lag, mapqual), [form % (half, 0)] + ([form % (0, 1)] if heavy else []), heavy=heavy, half=half)


# ---------------------------------------------------------------------------------------------------------------
# fragment-length histogram: k_frag_tiles<NT, merge, ltab>
# ---------------------------------------------------------------------------------------------------------------
FRAG_SHAPES = deck.FRAG_SHAPES         # ltab -> (tlen_filter, len_bin); tests/test_forms_deck_cpu.py: both island groups count in each
# (layout, merging form, ltab, midpoint rule)
FRAG = [("packed", m, lt, mid) for m in (False, True) for lt, mid in ((0, False), (1, True))] + \
       [("packed", False, 1, False), ("packed", True, 0, True), ("packed_noshort", False, 1, True), ("nopack", False, 1, False),
        ("nopack", True, 0, True)]


@pytest.mark.parametrize("layout,merge,ltab,mid", FRAG)
@pytest.mark.parametrize("nt", NTS)
def test_frag(gpu, nt, layout, merge, ltab, mid):
    from bamsignals_amd.device import FragPlan
    tf, len_bin = FRAG_SHAPES[ltab]
    _case(gpu, layout, lambda *a: FragPlan(*a, _params("frag", tlen_filter=tf, pe_mid=mid, threads=nt), len_bin),
          deck.expected_frag(tf, len_bin, mid), [f"k_frag_tiles<{nt},merge={int(merge)},ltab={ltab}>"],
          env={"BAMSIGNALS_FRAG_FORM": "merge" if merge else "plain"})


# ---------------------------------------------------------------------------------------------------------------
# the per-base reductions: what a (layout, signal, word) runs as
# ---------------------------------------------------------------------------------------------------------------
def _hist_kind(layout, signal, word):
    """(the main launch's kind, the wide launch's kind, half form, mapqual)"""
    if signal == "coverage":
        return "kHistCover", "kHistCover", False, 0
    half, mapqual = _reads_kind(layout, word)
    return ("kHistEndsHalf" if half else "kHistEnds"), "kHistEnds", half, mapqual


def _run_tiles(case):
    """runs of three tiles for the second round's cases with the smallest tiles and no heavy ones: a range of the deck has
    up to 257 such tiles and up to three ranges share a run, so runs end inside ranges and ranges change inside runs"""
    return "3" if case[4] <= 18 and not case[5] else None


def _kinds_of(cases):
    """the cases by what they run as: coverage, 5' ends from the 16-bit columns (half), 5' ends from 4-byte words"""
    out = {"coverage": [], "half": [], "word": []}
    for c in cases:
        out["coverage" if c[1] == "coverage" else "half" if _hist_kind(c[0], c[1], c[2])[2] else "word"].append(c)
    return out


# (layout, signal, word form, ss, tile_cells, heavy): tiles of 16, 20 (18, rounded up), 256 and 2,048 cells
TILES = [("packed", "coverage", False, False, 18, False), ("nopack", "coverage", False, False, 2048, False),
         ("packed", "coverage", False, False, 256, True), ("packed_noshort", "coverage", False, False, 16, True),
         ("packed", "ends", False, False, 16, False), ("packed", "ends", False, True, 2048, False),
         ("packed", "ends", False, True, 18, False), ("packed", "ends", False, False, 256, False),
         ("packed_noshort", "ends", False, True, 256, False), ("packed_noshort", "ends", False, False, 18, False),
         ("packed", "ends", True, True, 18, False), ("nopack", "ends", False, False, 256, False),
         ("nopack", "ends", False, True, 2048, False),
         ("packed", "ends", False, True, 2048, True), ("nopack", "ends", False, False, 16, True)]


# ---------------------------------------------------------------------------------------------------------------
# depth histogram: k_hist_tiles<NT, kind, wide, form>
# ---------------------------------------------------------------------------------------------------------------
# max_value 1 (everything at or above 1 lands in the top row) and 50; the plain and the merging consumer
HIST = [c + (v, f) for i, c in enumerate(TILES) for v, f in (((1, 50)[i % 2], (i // 2) % 2), ((50, 1)[i % 2], 1 - (i // 2) % 2))]


def test_hist_cases_cover_the_parameters():
    for kind, mine in _kinds_of(HIST).items():
        assert {(c[6], c[7]) for c in mine} == {(1, 0), (1, 1), (50, 0), (50, 1)}, kind
        assert {c[4] for c in mine} == {16, 18, 256, 2048}, kind
        if kind != "coverage":
            assert {c[3] for c in mine} == {False, True}
    assert {(c[1], c[7]) for c in HIST if c[5]} == {("coverage", 0), ("coverage", 1), ("ends", 0), ("ends", 1)}


@pytest.mark.parametrize("layout,signal,word,ss,tile,heavy,max_value,form", HIST)
@pytest.mark.parametrize("nt", NTS)
def test_hist(gpu, nt, layout, signal, word, ss, tile, heavy, max_value, form):
    from bamsignals_amd.device import HistPlan
    kind, wide_kind, half, mapqual = _hist_kind(layout, signal, word)
    name = f"k_hist_tiles<{nt},%s,wide=%d,form={form}>"
    _case(gpu, layout, lambda *a: HistPlan(*a, _params(signal, ss, mapqual=mapqual, tile_cells=tile, threads=nt), max_value),
          deck.expected_hist(signal, ss, max_value, mapqual), [name % (kind, 0)] + ([name % (wide_kind, 1)] if heavy else []),
          env={"BAMSIGNALS_HIST_FORM": "merge" if form else "plain"}, heavy=heavy, half=half)


# ---------------------------------------------------------------------------------------------------------------
# per-range summaries: k_summary_tiles<NT, kind, wide>
# ---------------------------------------------------------------------------------------------------------------
# no thresholds and eight, in turn; runs of three tiles for some cases of every kind
SUMMARY = [c + (((), deck.THRESHOLDS)[i % 2], None) for i, c in enumerate(TILES)] + \
          [c + ((deck.THRESHOLDS, ())[i % 2], _run_tiles(c)) for i, c in enumerate(TILES)]


def test_summary_cases_cover_the_parameters():
    for kind, mine in _kinds_of(SUMMARY).items():
        assert {len(c[6]) for c in mine} == {0, 8}, kind
        assert {c[4] for c in mine} == {16, 18, 256, 2048}, kind
        assert any(c[7] for c in mine) and any(c[5] for c in mine), kind
    assert {c[0] for c in _kinds_of(SUMMARY)["half"] if c[7]} == {"packed", "packed_noshort"}


@pytest.mark.parametrize("layout,signal,word,ss,tile,heavy,thresholds,run_tiles", SUMMARY)
@pytest.mark.parametrize("nt", NTS)
def test_summary(gpu, nt, layout, signal, word, ss, tile, heavy, thresholds, run_tiles):
    from bamsignals_amd.device import SummaryPlan
    kind, wide_kind, half, mapqual = _hist_kind(layout, signal, word)
    name = f"k_summary_tiles<{nt},%s,wide=%d>"
    _case(gpu, layout, lambda *a: SummaryPlan(*a, _params(signal, ss, mapqual=mapqual, tile_cells=tile, threads=nt), thresholds),
          deck.expected_summary(signal, ss, thresholds, mapqual), [name % (kind, 0)] + ([name % (wide_kind, 1)] if heavy else []),
          env={"BAMSIGNALS_SUMMARY_RUN_TILES": run_tiles}, heavy=heavy, half=half)


# ---------------------------------------------------------------------------------------------------------------
# scaled regions: k_scaled_tiles<NT, kind, wide, seg>
# ---------------------------------------------------------------------------------------------------------------
# 1, 20 and 2,048 bins (more bins than most ranges have bases), the plain and the segmented consumer (the wide form has
# the plain one alone), runs of three tiles for some
SCALED = [c + ((1, 20, 2048)[i % 3], i % 2, None) for i, c in enumerate(TILES)] + \
         [c + ((20, 2048, 1)[i % 3], 1 - i % 2, _run_tiles(c)) for i, c in enumerate(TILES)]


def test_scaled_cases_cover_the_parameters():
    for kind, mine in _kinds_of(SCALED).items():
        assert {c[6] for c in mine} == {1, 20, 2048} and {c[7] for c in mine} == {0, 1}, kind
        assert any(c[8] for c in mine) and any(c[5] for c in mine), kind


@pytest.mark.parametrize("layout,signal,word,ss,tile,heavy,n_bins,seg,run_tiles", SCALED)
@pytest.mark.parametrize("nt", NTS)
def test_scaled(gpu, nt, layout, signal, word, ss, tile, heavy, n_bins, seg, run_tiles):
    from bamsignals_amd.device import ScaledPlan
    kind, wide_kind, half, mapqual = _hist_kind(layout, signal, word)
    name = f"k_scaled_tiles<{nt},%s,wide=%d,seg=%d>"
    _case(gpu, layout, lambda *a: ScaledPlan(*a, _params(signal, ss, mapqual=mapqual, tile_cells=tile, threads=nt), n_bins),
          deck.expected_scaled(signal, ss, n_bins, mapqual), [name % (kind, 0, seg)] + ([name % (wide_kind, 1, 0)] if heavy else []),
          env={"BAMSIGNALS_SCALED_SEGMENTED": str(seg), "BAMSIGNALS_SCALED_RUN_TILES": run_tiles}, heavy=heavy, half=half)


# ---------------------------------------------------------------------------------------------------------------
# the whole list
# ---------------------------------------------------------------------------------------------------------------
def test_the_occupancy_queries_log_nothing(gpu):
    """making a plan asks tile_blocks_per_cu, which goes through the same selectors: only a run's launches are logged"""
    from bamsignals_amd.device import HistPlan
    from test_kernel_forms_gpu import _selected
    ctx, reads = gpu
    rg = deck.ranges()
    with _selected({}) as drain:
        plan = HistPlan(ctx, reads["packed"], rg["rid"], rg["loc"], rg["len"], rg["strand"], _params("ends", True, threads=64), 50)
        try:
            assert drain() == []
            plan.run_host()
            assert drain() == ["k_hist_tiles<64,kHistEndsHalf,wide=0,form=0>"]
        finally:
            plan.close()


def test_every_form_was_reached():
    """Runs after the matrix (pytest keeps a module's order): the forms the cases logged are exactly ALL_FORMS."""
    assert len(ALL_FORMS) == len(set(ALL_FORMS)) == 90
    per_kernel = {}
    for n in ALL_FORMS:
        per_kernel[n.split("<")[0]] = per_kernel.get(n.split("<")[0], 0) + 1
    assert per_kernel == {"k_xcorr_tiles": 9, "k_frag_tiles": 12, "k_hist_tiles": 30, "k_summary_tiles": 15, "k_scaled_tiles": 24}
    missing, unknown = sorted(set(ALL_FORMS) - SEEN), sorted(SEEN - set(ALL_FORMS))
    assert not missing and not unknown, dict(never_reached=missing, not_listed=unknown)
