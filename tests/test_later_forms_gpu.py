"""GPU: the kernel forms that came after tests/test_kernel_forms_gpu.py and tests/test_reduction_forms_gpu.py, run on
tests/forms_deck.py and compared with the C oracle exactly -- every form that capped_form (keepDup: k_capped_tiles, 18
instantiations), vplot_form (bamVPlot: k_vplot_tiles, 18) and, for a resized plan (fragLength), launch_mode and sum_form
(k_coverage, k_coverage_bins and k_sum_tiles with frag=1: 6 + 12 + 12 = 30) of csrc/kernels.hip can launch.  A case is
the two earlier modules': the call parameters and environment that select one form are set, the launch log is turned on
(bsig_debug_launch_log), the plan is made and run twice -- the first run looks its windows up in the kernel, the second
reads the kept ones --, both runs are compared with the deck's expected side (forms_deck.expected_capped / _capped_cover /
_vplot / _resized / _resized_sum), and the log must hold exactly the names the case lists.  Every family has a closing test
with the literal list of its names: a form nobody reached fails it, and so does a form nobody listed.

The layouts are test_reduction_forms_gpu.py's: `packed` (half forms read 16-bit columns), `packed_noshort`
(BAMSIGNALS_SHORT_HALF=0) and `nopack` (BAMSIGNALS_PACK=0, word forms only); on a packed layout mapqual=10 reaches a word
form.  BAMSIGNALS_HEAVY_READS=64 gives wide tiles (capped: a second launch of kHistEnds,wide=1) and the accumulate launch
of a resized plan.  What makes a case not vacuous -- cells above and below every cap, every branch of CappedCells::add,
the scratch rows of k_capped_scan, the V-plot's shapes -- is checked on the expected sides in tests/test_forms_deck_cpu.py,
which reads the case tables of this module."""
import numpy as np
import pytest

import forms_deck as deck
from test_kernel_forms_gpu import COV_BINS, _selected
from test_reduction_forms_gpu import BYTES_PER_VISIT, NTS, _env, _reads_kind, gpu  # noqa: F401  (gpu: the reads in three layouts)

pytestmark = pytest.mark.gpu

SEEN_CAPPED, SEEN_VPLOT, SEEN_RESIZED = set(), set(), set()      # the names each family's cases logged

CAPPED_FORMS = (
    "k_capped_tiles<64,kHistEndsHalf,wide=0,binned=0>",
    "k_capped_tiles<64,kHistEndsHalf,wide=0,binned=1>",
    "k_capped_tiles<64,kHistEnds,wide=0,binned=0>",
    "k_capped_tiles<64,kHistEnds,wide=0,binned=1>",
    "k_capped_tiles<64,kHistEnds,wide=1,binned=0>",
    "k_capped_tiles<64,kHistEnds,wide=1,binned=1>",
    "k_capped_tiles<128,kHistEndsHalf,wide=0,binned=0>",
    "k_capped_tiles<128,kHistEndsHalf,wide=0,binned=1>",
    "k_capped_tiles<128,kHistEnds,wide=0,binned=0>",
    "k_capped_tiles<128,kHistEnds,wide=0,binned=1>",
    "k_capped_tiles<128,kHistEnds,wide=1,binned=0>",
    "k_capped_tiles<128,kHistEnds,wide=1,binned=1>",
    "k_capped_tiles<256,kHistEndsHalf,wide=0,binned=0>",
    "k_capped_tiles<256,kHistEndsHalf,wide=0,binned=1>",
    "k_capped_tiles<256,kHistEnds,wide=0,binned=0>",
    "k_capped_tiles<256,kHistEnds,wide=0,binned=1>",
    "k_capped_tiles<256,kHistEnds,wide=1,binned=0>",
    "k_capped_tiles<256,kHistEnds,wide=1,binned=1>",
)

VPLOT_FORMS = (
    "k_vplot_tiles<64,global=0,ltab=1,merge=0>",
    "k_vplot_tiles<64,global=0,ltab=1,merge=1>",
    "k_vplot_tiles<64,global=0,ltab=0,merge=0>",
    "k_vplot_tiles<64,global=0,ltab=0,merge=1>",
    "k_vplot_tiles<64,global=1,ltab=1,merge=0>",
    "k_vplot_tiles<64,global=1,ltab=1,merge=1>",
    "k_vplot_tiles<128,global=0,ltab=1,merge=0>",
    "k_vplot_tiles<128,global=0,ltab=1,merge=1>",
    "k_vplot_tiles<128,global=0,ltab=0,merge=0>",
    "k_vplot_tiles<128,global=0,ltab=0,merge=1>",
    "k_vplot_tiles<128,global=1,ltab=1,merge=0>",
    "k_vplot_tiles<128,global=1,ltab=1,merge=1>",
    "k_vplot_tiles<256,global=0,ltab=1,merge=0>",
    "k_vplot_tiles<256,global=0,ltab=1,merge=1>",
    "k_vplot_tiles<256,global=0,ltab=0,merge=0>",
    "k_vplot_tiles<256,global=0,ltab=0,merge=1>",
    "k_vplot_tiles<256,global=1,ltab=1,merge=0>",
    "k_vplot_tiles<256,global=1,ltab=1,merge=1>",
)

RESIZED_FORMS = (
    "k_coverage<64,pre=2,res=0,frag=1> acc=0",
    "k_coverage<64,pre=2,res=1,frag=1> acc=0",
    "k_coverage<64,pre=2,res=0,frag=1> acc=1",
    "k_coverage<128,pre=2,res=0,frag=1> acc=0",
    "k_coverage<128,pre=2,res=1,frag=1> acc=0",
    "k_coverage<128,pre=2,res=0,frag=1> acc=1",
    "k_coverage<256,pre=2,res=0,frag=1> acc=0",
    "k_coverage<256,pre=2,res=1,frag=1> acc=0",
    "k_coverage<256,pre=2,res=0,frag=1> acc=1",
    "k_coverage_bins<64,pre=2,res=0,ss=0,frag=1> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=1,ss=0,frag=1> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=0,ss=0,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=1,ss=0,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=0,ss=0,frag=1> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=1,ss=0,frag=1> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=0,ss=0,frag=1> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=1,ss=0,frag=1> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=0,ss=0,frag=1> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=1,ss=0,frag=1> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=0,ss=0,frag=1> acc=1 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=0,ss=1,frag=1> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=1,ss=1,frag=1> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=0,ss=1,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=1,ss=1,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=0,ss=1,frag=1> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=1,ss=1,frag=1> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=0,ss=1,frag=1> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=1,ss=1,frag=1> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=0,ss=1,frag=1> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=1,ss=1,frag=1> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=0,ss=1,frag=1> acc=1 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=0,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=1,ss=0,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=0,frag=1> acc=1 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=1,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=1,ss=1,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=1,frag=1> acc=1 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=0,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=1,ss=0,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=0,frag=1> acc=1 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=1,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=1,ss=1,frag=1> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=1,frag=1> acc=1 cov_reps=8",
    "k_sum_tiles<nw=1,kSumCover,ss=0,half=0,res=0,frag=1>",
    "k_sum_tiles<nw=1,kSumCover,ss=0,half=0,res=1,frag=1>",
    "k_sum_tiles<nw=1,kSumCoverSS,ss=1,half=0,res=0,frag=1>",
    "k_sum_tiles<nw=1,kSumCoverSS,ss=1,half=0,res=1,frag=1>",
    "k_sum_tiles<nw=2,kSumCover,ss=0,half=0,res=0,frag=1>",
    "k_sum_tiles<nw=2,kSumCover,ss=0,half=0,res=1,frag=1>",
    "k_sum_tiles<nw=2,kSumCoverSS,ss=1,half=0,res=0,frag=1>",
    "k_sum_tiles<nw=2,kSumCoverSS,ss=1,half=0,res=1,frag=1>",
    "k_sum_tiles<nw=4,kSumCover,ss=0,half=0,res=0,frag=1>",
    "k_sum_tiles<nw=4,kSumCover,ss=0,half=0,res=1,frag=1>",
    "k_sum_tiles<nw=4,kSumCoverSS,ss=1,half=0,res=0,frag=1>",
    "k_sum_tiles<nw=4,kSumCoverSS,ss=1,half=0,res=1,frag=1>",
)


# ---------------------------------------------------------------------------------------------------------------
# one case
# ---------------------------------------------------------------------------------------------------------------
def _case(gpu, layout, seen, make, rg, want, expect, env=None, heavy=False, half=False, offsets=None, form=None):
    """One case: make(ctx, reads, range arrays) -> the plan, made with `env` set; nothing is logged before the first run;
    both runs against `want`, the log against `expect`, heavy tiles iff asked for; for a half form the bytes a visit of
    classes 0 / 1 and of the packed class reads; offsets / form: the plan's, where the kind has them."""
    ctx, reads = gpu
    with _selected({}, heavy=heavy) as drain, _env(env or {}):
        plan = make(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"])
        try:
            made = drain()
            first, second, st = plan.run_host().copy(), plan.run_host().copy(), plan.stats()
            if offsets is not None:
                assert np.array_equal(plan.offsets, offsets)
            if form is not None:
                assert plan.form == form, (plan.form, form)
        finally:
            plan.close()
        names = drain()
    seen.update(names)
    want = np.asarray(want)
    assert made == []
    assert want.any() and want.dtype in (np.int32, np.int64)
    assert first.shape == want.shape, (first.shape, want.shape)
    assert np.array_equal(first, want), (names, int(np.sum(first != want)), np.argwhere(first != want)[:8].tolist())
    assert np.array_equal(second, want), (names, int(np.sum(second != want)), np.argwhere(second != want)[:8].tolist())
    assert set(names) == set(expect), (names, expect)
    assert (st["heavy_tiles"] > 0) == heavy
    if half:
        assert (st["bytes_per_visit_short"], st["bytes_per_visit_packed"]) == BYTES_PER_VISIT[layout], layout
        assert st["visits_short"] > 0
    return st


def _closing(all_forms, seen, n_instantiations):
    assert len(all_forms) == len(set(all_forms))
    assert len({n.split("> ")[0] for n in all_forms}) == n_instantiations
    missing, unknown = sorted(set(all_forms) - seen), sorted(seen - set(all_forms))
    assert not missing and not unknown, dict(never_reached=missing, not_listed=unknown)


# ---------------------------------------------------------------------------------------------------------------
# keepDup: k_capped_tiles<NT, kHistEnds / kHistEndsHalf, wide, binned>
# ---------------------------------------------------------------------------------------------------------------
CAPPED_TILES = (16, 18, 256, 2048)                       # 16, 20 (18, rounded up), 256 and 2,048 cells
CAPPED_KS = (1, 2, 5)
# (binsize, ss): bins of one base (the tile stores its cells: binned=0), bins of 7 and 274 bases and bamCount's one bin
CAPPED_BINS = ((1, False), (1, True), (7, False), (7, True), (274, False), (274, True), (-1, False), (-1, True))
# kind -> (layout, word form on a packed layout)
CAPPED_KINDS = {"half": ("packed", False), "half_noshort": ("packed_noshort", False), "word_nopack": ("nopack", False),
                "word_packed": ("packed", True)}


def _capped_cases():
    """(layout, word, binsize, ss, tile_cells, k, shift, run_tiles, heavy): every (binsize, ss) of every kind in rounds
    that move the tile size, the cap and the shift on, then the wide cases"""
    out = []
    for ki, (kind, rounds) in enumerate((("half", (0, 1)), ("half_noshort", (0,)), ("word_nopack", (0, 1)), ("word_packed", (1,)))):
        layout, word = CAPPED_KINDS[kind]
        for rnd in rounds:
            for i, (binsize, ss) in enumerate(CAPPED_BINS):
                tile = CAPPED_TILES[(i + ki + 2 * rnd) % 4]
                out.append((layout, word, binsize, ss, tile, CAPPED_KS[(i + ki + rnd) % 3], 75 if (i + rnd) % 4 == 1 else 0,
                            "3" if tile <= 18 and i % 2 == 1 else None, False))
    # wide tiles (BAMSIGNALS_HEAVY_READS=64): every kind with bins of one base and with wider ones, a shift among them
    out += [("packed", False, 1, True, 256, 2, 0, None, True), ("packed", False, 7, False, 2048, 1, 75, None, True),
            ("packed_noshort", False, -1, True, 256, 5, 0, None, True), ("packed_noshort", False, 1, False, 2048, 2, 0, None, True),
            ("nopack", False, 1, False, 2048, 5, 75, None, True), ("nopack", False, 274, True, 256, 2, 0, None, True),
            ("packed", True, 1, True, 2048, 1, 0, None, True), ("packed", True, 7, True, 256, 2, 75, None, True)]
    return out


CAPPED = _capped_cases()
# the coverage form (layout, word, frag_len, binsize, ss, tile_cells, k, heavy): per-base tiles with strands whatever the
# result's bins, then k_capped_scan and k_capped_cover; frag_len 1 makes a range's scratch row as long as the range
CAPPED_COVER = [("packed", False, 1, 1, False, 256, 1, False), ("packed", False, 36, 50, True, 2048, 2, False),
                ("packed", False, 200, 1, True, 18, 5, False), ("packed_noshort", False, 1, 50, True, 2048, 2, False),
                ("packed_noshort", False, 200, 1, False, 16, 1, False), ("nopack", False, 1, 1, True, 2048, 5, False),
                ("nopack", False, 36, 1, False, 18, 1, False), ("nopack", False, 200, 50, False, 256, 2, False),
                ("packed", True, 1, 50, False, 16, 2, False), ("packed", True, 36, 1, True, 256, 5, False),
                ("packed", False, 36, 1, True, 256, 2, True), ("nopack", False, 200, 50, False, 2048, 1, True)]


def capped_kind(layout, word):
    return "word_packed" if word else {"packed": "half", "packed_noshort": "half", "nopack": "word_nopack"}[layout]


def test_capped_cases_cover_the_parameters():
    by_kind = {}
    for c in CAPPED:
        by_kind.setdefault(capped_kind(c[0], c[1]), []).append(c)
    assert set(by_kind) == {"half", "word_nopack", "word_packed"}
    assert {c[0] for c in by_kind["half"]} == {"packed", "packed_noshort"}
    for kind, mine in by_kind.items():
        assert {(c[2], c[3]) for c in mine} == set(CAPPED_BINS), kind
        assert {c[4] for c in mine} == set(CAPPED_TILES), kind
        stored = {c[4] for c in mine if c[2] == 1}                  # bins of one base: a small tile and a large one at least
        assert min(stored) <= 18 and max(stored) >= 256 and {c[4] for c in mine if c[2] != 1} == set(CAPPED_TILES), kind
        assert {c[5] for c in mine} == set(CAPPED_KS) and {c[6] for c in mine} == {0, 75}, kind
        assert any(c[7] and c[4] <= 18 for c in mine), kind                      # runs of three small tiles
        assert {c[2] == 1 for c in mine if c[8]} == {False, True}, kind         # wide: binned 0 and 1
    assert any(c[8] and c[6] == 75 for c in CAPPED)
    cover = {}
    for c in CAPPED_COVER:
        cover.setdefault(capped_kind(c[0], c[1]), []).append(c)
    assert set(cover) == set(by_kind)
    assert {c[2] for c in CAPPED_COVER} == {1, 36, 200} and {(c[3], c[4]) for c in CAPPED_COVER} == {(1, False), (1, True), (50, False), (50, True)}
    assert {c[5] for c in CAPPED_COVER} == set(CAPPED_TILES) and any(c[7] for c in CAPPED_COVER)


def _capped_names(nt, layout, word, binned, heavy):
    half, mapqual = _reads_kind(layout, word)
    name = f"k_capped_tiles<{nt},%s,wide=%d,binned={int(binned)}>"
    return [name % ("kHistEndsHalf" if half else "kHistEnds", 0)] + ([name % ("kHistEnds", 1)] if heavy else []), half, mapqual


@pytest.mark.parametrize("layout,word,binsize,ss,tile,k,shift,run_tiles,heavy", CAPPED)
@pytest.mark.parametrize("nt", NTS)
def test_capped(gpu, nt, layout, word, binsize, ss, tile, k, shift, run_tiles, heavy):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import CappedPlan, make_params
    names, half, mapqual = _capped_names(nt, layout, word, binsize != 1, heavy)
    want, off = deck.expected_capped(k, binsize, ss, shift, mapqual)
    mode = _lib.MODE_COUNT if binsize < 0 else _lib.MODE_PROFILE
    _case(gpu, layout, SEEN_CAPPED,
          lambda *a: CappedPlan(*a, make_params(mode, binsize=binsize, ss=ss, shift=shift, mapqual=mapqual, tile_cells=tile, threads=nt), k),
          deck.ranges(), want, names, env={"BAMSIGNALS_CAPPED_RUN_TILES": run_tiles}, heavy=heavy, half=half, offsets=off)


@pytest.mark.parametrize("layout,word,frag_len,binsize,ss,tile,k,heavy", CAPPED_COVER)
@pytest.mark.parametrize("nt", NTS)
def test_capped_coverage(gpu, nt, layout, word, frag_len, binsize, ss, tile, k, heavy):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import CappedPlan, make_params
    names, half, mapqual = _capped_names(nt, layout, word, False, heavy)
    want, off = deck.expected_capped_cover(k, frag_len, binsize, ss, mapqual)
    _case(gpu, layout, SEEN_CAPPED,
          lambda *a: CappedPlan(*a, make_params(_lib.MODE_COVERAGE_EX, binsize=binsize, ss=ss, mapqual=mapqual, tile_cells=tile, threads=nt),
                                k, frag_len),
          deck.ranges(), want, names, env={"BAMSIGNALS_CAPPED_RUN_TILES": None}, heavy=heavy, half=half, offsets=off)


def test_every_capped_form_was_reached():
    """Runs after the cases (pytest keeps a module's order): the forms they logged are exactly CAPPED_FORMS."""
    _closing(CAPPED_FORMS, SEEN_CAPPED, 18)


# ---------------------------------------------------------------------------------------------------------------
# bamVPlot: k_vplot_tiles<NT, global, ltab, merge>
# ---------------------------------------------------------------------------------------------------------------
# which -> (shape of forms_deck.VPLOT_SHAPES, environment, global, ltab).  The small table lies in LDS with its filter
# table behind it; under a budget of 14 KiB (14,336 bytes) its 3,526 counters still fit and the 512 bytes of the filter
# table no longer do; BAMSIGNALS_VPLOT_FORM=global sends it to global atomics.  The other three are the library's own
# choice at the device's 160 KiB: a table of exactly 40,960 counters leaves the filter table no room, one row fewer does,
# one row more is the global form.
VPLOT_WHICH = {"small": ("small", {}, 0, 1), "small_14k": ("small", {"BAMSIGNALS_VPLOT_LDS_KIB": "14"}, 0, 0),
               "small_global": ("small", {"BAMSIGNALS_VPLOT_FORM": "global"}, 1, 1),
               "budget": ("budget", {}, 0, 0), "below": ("below", {}, 0, 1), "above": ("above", {}, 1, 1)}


def _vplot_cases():
    """(layout, which, merge, midpoint, tile_cells, run_tiles, mapqual): tiles of 2,048 bases make one tile an island, so
    that a window is exactly the island's m reads; tiles of 256 cut every range in eight"""
    out = []
    for j, which in enumerate(VPLOT_WHICH):
        for merge in (0, 1):
            mid, tile = bool((j + merge) % 2), (2048, 256)[j % 2]
            out.append(("packed", which, merge, mid, tile, "3" if (j + merge) % 3 == 0 else None, 0))
            out.append(("packed", which, merge, not mid, (2048, 256)[(j + 1) % 2], None, 0))
            out.append(("nopack", which, merge, mid, (2048, 256)[(j + merge) % 2], "3" if (j + merge) % 3 == 1 else None, 0))
    out += [("packed_noshort", "small", 0, True, 256, None, 0), ("packed_noshort", "budget", 1, False, 2048, None, 0),
            ("packed", "small", 0, True, 2048, None, 10)]
    return out


VPLOT = _vplot_cases()


def test_vplot_cases_cover_the_parameters():
    for layout in ("packed", "nopack"):
        mine = [c for c in VPLOT if c[0] == layout]
        assert {(c[1], c[2]) for c in mine} == {(w, m) for w in VPLOT_WHICH for m in (0, 1)}, layout
        assert {(c[1], c[4]) for c in mine} == {(w, t) for w in VPLOT_WHICH for t in (256, 2048)}, layout
        assert {(c[1], c[3]) for c in mine} >= {(w, m) for w in ("small", "budget", "below", "above") for m in (False, True)}, layout
        assert any(c[5] for c in mine), layout
    assert any(c[0] == "packed_noshort" for c in VPLOT) and any(c[6] for c in VPLOT)


@pytest.mark.parametrize("layout,which,merge,midpoint,tile,run_tiles,mapqual", VPLOT)
@pytest.mark.parametrize("nt", NTS)
def test_vplot(gpu, nt, layout, which, merge, midpoint, tile, run_tiles, mapqual):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import VplotPlan, make_params
    shape, env, glob, ltab = VPLOT_WHICH[which]
    tf, len_bin, binsize = deck.VPLOT_SHAPES[shape]
    want = deck.expected_vplot(tf, len_bin, binsize, midpoint, mapqual)
    assert want.size == deck.VPLOT_CELLS[shape]
    env = {"BAMSIGNALS_VPLOT_LDS_KIB": None, "BAMSIGNALS_VPLOT_FORM": None, "BAMSIGNALS_VPLOT_FLUSH_READS": None, **env,
           "BAMSIGNALS_VPLOT_MERGE": "1" if merge else None, "BAMSIGNALS_VPLOT_RUN_TILES": run_tiles}
    st = _case(gpu, layout, SEEN_VPLOT,
               lambda *a: VplotPlan(*a, make_params(_lib.MODE_PROFILE, tlen_filter=tf, pe_mid=midpoint, binsize=binsize, requiredF=66,
                                                    mapqual=mapqual, tile_cells=tile, threads=nt), len_bin),
               deck.sum_ranges(), want, [f"k_vplot_tiles<{nt},global={glob},ltab={ltab},merge={merge}>"], env=env, form=glob)
    assert st["cells"] == want.size and st["n_items"] == len(deck.sum_ranges()["len"]) * (2048 // tile)
    if layout == "packed":
        assert st["bytes_per_visit_packed"] == 8 and st["visits_packed"] > 0      # the word and its tlen
    if layout == "nopack":
        assert st["visits_packed"] == 0


def test_every_vplot_form_was_reached():
    _closing(VPLOT_FORMS, SEEN_VPLOT, 18)


# ---------------------------------------------------------------------------------------------------------------
# fragLength: k_coverage, k_coverage_bins and k_sum_tiles with frag=1
# ---------------------------------------------------------------------------------------------------------------
RESIZED_L = (36, 5000)
RESIZED_LAYOUTS = ("packed", "nopack")


def _resized_case(gpu, layout, L, pset, expect, tile_cells, threads, heavy=False):
    from bamsignals_amd.device import Plan, make_params
    mode, a = deck.gpu_args(pset)
    want, off = deck.expected_resized(L, pset)
    st = _case(gpu, layout, SEEN_RESIZED, lambda *r: Plan(*r, make_params(mode, tile_cells=tile_cells, threads=threads, **a), frag_len=L),
               deck.ranges(), want, expect, heavy=heavy, offsets=off)
    # no tlen column is read for the length: a packed visit is its word
    assert st["bytes_per_visit_packed"] == 4 and (st["visits_packed"] > 0) == (layout == "packed")


@pytest.mark.parametrize("tile,heavy", [(256, False), (2048, False), (256, True)])
@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("layout", RESIZED_LAYOUTS)
@pytest.mark.parametrize("L", RESIZED_L)
def test_resized_coverage(gpu, L, layout, nt, tile, heavy):
    form = f"k_coverage<{nt},pre=2,res=%d,frag=1> acc=%d"
    _resized_case(gpu, layout, L, "cover", [form % (0, 0), form % (1, 0)] + ([form % (0, 1)] if heavy else []), tile, nt, heavy)


@pytest.mark.parametrize("pset,tile,cells,reps", COV_BINS)
@pytest.mark.parametrize("layout", RESIZED_LAYOUTS)
@pytest.mark.parametrize("L", RESIZED_L)
def test_resized_coverage_bins_replicas(gpu, L, layout, pset, tile, cells, reps):
    ss = int(pset.endswith("ss1"))
    form = f"k_coverage_bins<64,pre=2,res=%d,ss={ss},frag=1> acc=0 cov_reps={reps}"
    _resized_case(gpu, layout, L, pset, [form % 0, form % 1], tile, 64)


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("layout", RESIZED_LAYOUTS)
@pytest.mark.parametrize("L", RESIZED_L)
def test_resized_coverage_bins_workgroups(gpu, L, layout, nt, ss, heavy):
    form = f"k_coverage_bins<{nt},pre=2,res=%d,ss={int(ss)},frag=1> acc=%d cov_reps=8"
    _resized_case(gpu, layout, L, f"bins2_ss{int(ss)}", [form % (0, 0), form % (1, 0)] + ([form % (0, 1)] if heavy else []),
                  64 if ss else 124, nt, heavy)


@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("layout", RESIZED_LAYOUTS)
@pytest.mark.parametrize("L", RESIZED_L)
def test_resized_sum_tiles(gpu, L, layout, ss, nw):
    """1, 2 and 4 tiles in flight per workgroup; 256-cell tiles, so that the 2,048-bp ranges have eight of them"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import SumPlan, make_params
    p = make_params(_lib.MODE_COVERAGE_EX, binsize=1, ss=True, tile_cells=256, threads=64 * nw) if ss else \
        make_params(_lib.MODE_COVERAGE, tile_cells=256, threads=64 * nw)
    form = f"k_sum_tiles<nw={nw},{'kSumCoverSS' if ss else 'kSumCover'},ss={int(ss)},half=0,res=%d,frag=1>"
    _case(gpu, layout, SEEN_RESIZED, lambda *r: SumPlan(*r, p, frag_len=L), deck.sum_ranges(), deck.expected_resized_sum(L, ss),
          [form % 0, form % 1])


def test_every_resized_form_was_reached():
    _closing(RESIZED_FORMS, SEEN_RESIZED, 30)


# ---------------------------------------------------------------------------------------------------------------
# the log
# ---------------------------------------------------------------------------------------------------------------
def test_making_the_plans_logs_nothing(gpu):
    """making a plan asks tile_blocks_per_cu, which goes through the same selectors: only a run's launches are logged"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import CappedPlan, Plan, SumPlan, VplotPlan, make_params
    ctx, reads = gpu
    rg, srg = deck.ranges(), deck.sum_ranges()
    a = (ctx, reads["packed"], rg["rid"], rg["loc"], rg["len"], rg["strand"])
    s = (ctx, reads["packed"], srg["rid"], srg["loc"], srg["len"], srg["strand"])
    tf, len_bin, binsize = deck.VPLOT_SHAPES["small"]
    makers = (
        (lambda: CappedPlan(*a, make_params(_lib.MODE_PROFILE, binsize=7, ss=True, threads=64), 2), "k_capped_tiles<64,kHistEndsHalf,wide=0,binned=1>"),
        (lambda: CappedPlan(*a, make_params(_lib.MODE_COVERAGE_EX, ss=True, threads=64), 2, 36), "k_capped_tiles<64,kHistEndsHalf,wide=0,binned=0>"),
        (lambda: VplotPlan(*s, make_params(_lib.MODE_PROFILE, tlen_filter=tf, pe_mid=True, binsize=binsize, requiredF=66, threads=64), len_bin),
         "k_vplot_tiles<64,global=0,ltab=1,merge=0>"),
        (lambda: Plan(*a, make_params(_lib.MODE_COVERAGE, threads=64), frag_len=36), "k_coverage<64,pre=2,res=0,frag=1> acc=0"),
        (lambda: SumPlan(*s, make_params(_lib.MODE_COVERAGE, tile_cells=256, threads=64), frag_len=36),
         "k_sum_tiles<nw=1,kSumCover,ss=0,half=0,res=0,frag=1>"))
    with _selected({}) as drain, _env({"BAMSIGNALS_VPLOT_LDS_KIB": None, "BAMSIGNALS_VPLOT_FORM": None, "BAMSIGNALS_VPLOT_MERGE": None}):
        for make, name in makers:
            plan = make()
            try:
                assert drain() == []
                plan.run_host()
                assert drain() == [name]
            finally:
                plan.close()
