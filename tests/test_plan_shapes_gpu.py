"""GPU: the plans that plan creation makes, against a table RECORDED from the library as it was before plan creation was
cut into stages (csrc/planmath.h, runtime.hip: plan_create_impl).  A case makes one plan on tests/forms_deck.py's reads
and records what the ABI shows of it: every field of bsig_plan_get_stats before the first run, the plan's cells and the
last entry of its offsets, the kind's *_runs count where there is one, the launch log of the first and of the second
run, and a CRC of the result bytes.  The library under test must reproduce the table exactly: the same tiles (n_items,
visits, streamed, algorithmic_bytes), the same heavy tiles, the same runs, the same kernel forms, the same result.

The cases: every PARAM_SETS and SUM_SETS entry at the deck's ranges; one plan of each reduction kind; a resized
coverage plan; an overlap plan with a caller's tile_cells; a profile with binsize 8193 (wide bins); a count plan with a
range of 40,000 bases; and four plans made under BAMSIGNALS_HEAVY_READS=64, so that slices and walked-whole tiles
occur on the deck's small islands.

`python tests/test_plan_shapes_gpu.py` prints the table of the library that BSIG_LIB_PATH names; it uses no entry
point that the library before the stages lacks."""
import contextlib
import ctypes
import os
import pprint
import zlib

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository on sys.path when this file runs as a script)
import forms_deck as deck

pytestmark = pytest.mark.gpu

HEAVY = {"BAMSIGNALS_HEAVY_READS": "64"}
# what a plan's shape depends on besides its arguments: read when the plan is made, so unset while a case makes its own
PLAN_ENV = ("BAMSIGNALS_HEAVY_READS", "BAMSIGNALS_OVERLAP_QUAD", "BAMSIGNALS_SUM_RUN_TILES", "BAMSIGNALS_XCORR_RUN_TILES",
            "BAMSIGNALS_FRAG_RUN_TILES", "BAMSIGNALS_HIST_RUN_TILES", "BAMSIGNALS_SUMMARY_RUN_TILES", "BAMSIGNALS_SCALED_RUN_TILES",
            "BAMSIGNALS_FRAG_FLUSH_READS", "BAMSIGNALS_HIST_FLUSH_CELLS", "BAMSIGNALS_FRAG_FORM", "BAMSIGNALS_HIST_FORM",
            "BAMSIGNALS_SCALED_SEGMENTED", "BAMSIGNALS_CACHE_WINDOWS")


def _wide_ranges():
    """the deck's ranges behind three long ones, one per strand: bins and bamCount ranges wider than a tile's 16,384 bases"""
    rg = deck.ranges()
    head = dict(rid=[0, 1, 2], loc=[100, 5, 0], len=[40_000, 40_000, 20_000], strand=[1, -1, 0])
    return {k: np.concatenate([np.asarray(head[k], np.int32), rg[k]]) for k in rg}


def _one_long_range():
    return dict(rid=np.zeros(1, np.int32), loc=np.full(1, 100, np.int32), len=np.full(1, 40_000, np.int32), strand=np.ones(1, np.int32))


def _make(name):
    """(constructor(ctx, reads, rid, loc, len, strand), ranges, environment) of a case"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import FragPlan, HistPlan, Plan, ScaledPlan, SummaryPlan, SumPlan, XcorrPlan, make_params
    env = HEAVY if name.startswith("heavy_") else {}
    base = name[len("heavy_"):] if env else name
    if base in deck.PARAM_SETS:
        mode, a = deck.gpu_args(base)
        return (lambda *r: Plan(*r, make_params(mode, **a))), deck.ranges(), env
    if base in deck.SUM_SETS:
        mode, a = deck.gpu_args(base)
        return (lambda *r: SumPlan(*r, make_params(mode, **a))), deck.sum_ranges(), env
    ends = dict(binsize=1, ss=True)
    made = {
        "xcorr": lambda *r: XcorrPlan(*r, make_params(_lib.MODE_PROFILE, tile_cells=256, **ends), 200),
        "frag": lambda *r: FragPlan(*r, make_params(_lib.MODE_COUNT, binsize=-1, requiredF=66, tlen_filter=(100, 400)), 7),
        "hist": lambda *r: HistPlan(*r, make_params(_lib.MODE_PROFILE, tile_cells=256, **ends), 50),
        "summary": lambda *r: SummaryPlan(*r, make_params(_lib.MODE_COVERAGE, tile_cells=18), deck.THRESHOLDS),
        "scaled": lambda *r: ScaledPlan(*r, make_params(_lib.MODE_PROFILE, **ends), 20),
        "resized": lambda *r: Plan(*r, make_params(_lib.MODE_COVERAGE), frag_len=150),
        "overlap_tile": lambda *r: Plan(*r, make_params(_lib.MODE_OVERLAP_ANY, binsize=1, ss=True, tile_cells=100)),
        "wide_bins": lambda *r: Plan(*r, make_params(_lib.MODE_PROFILE, binsize=8193, ss=True)),
        "count_long": lambda *r: Plan(*r, make_params(_lib.MODE_COUNT, binsize=-1, ss=True)),
    }
    ranges = {"wide_bins": _wide_ranges, "count_long": _one_long_range}.get(base, deck.ranges)()
    return made[base], ranges, env


CASES = list(deck.PARAM_SETS) + list(deck.SUM_SETS) + ["xcorr", "frag", "hist", "summary", "scaled", "resized", "overlap_tile",
                                                       "wide_bins", "count_long", "heavy_half_ss1", "heavy_bins2_ss1",
                                                       "heavy_sum_half_ss0", "heavy_hist"]


@contextlib.contextmanager
def _env(values):
    old = {k: os.environ.pop(k, None) for k in PLAN_ENV}
    os.environ.update(values)
    try:
        yield
    finally:
        for k in PLAN_ENV:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


def record(ctx, reads, name):
    """what the ABI shows of the case's plan"""
    from bamsignals_amd import _lib
    lib = _lib.load()
    log = lib.bsig_debug_launch_log
    log.argtypes, log.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    buf = ctypes.create_string_buffer(65537)

    def drain():
        log(buf, len(buf))
        return buf.value.decode().splitlines()
    make, rg, env = _make(name)
    with _env(env):
        plan = make(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
    try:
        out = dict(stats=plan.stats(), cells=int(plan.cells), off_last=int(lib.bsig_plan_cells(plan._h)))
        if isinstance(getattr(plan, "runs", None), int):
            out["runs"] = plan.runs
        assert log(None, 1) >= 0
        try:
            first = plan.run_host().copy()
            out["log1"] = drain()
            second = plan.run_host().copy()
            out["log2"] = drain()
        finally:
            log(None, 0)
    finally:
        plan.close()
    assert np.array_equal(first, second), name
    out["crc"] = zlib.crc32(np.ascontiguousarray(first).tobytes())
    return out


@contextlib.contextmanager
def _resident():
    from bamsignals_amd.device import Context, Reads
    c = deck.reads()
    ctx = Context(0)
    with _env({}):
        reads = Reads(ctx, c["ref_len"], c["ref_off"], c["pos"], c["flag"], c["mapq"], c["tlen"], end=c["end"])
    try:
        yield ctx, reads
    finally:
        reads.close()
        ctx.close()


@pytest.fixture(scope="module")
def gpu():
    with _resident() as g:
        yield g


# ---- recorded from the library of the commit before the stages (see the module's docstring); not derived from the code under test
EXPECTED = {
    'half_ss0': {
        'stats': {'n_ranges': 490, 'n_items': 522, 'cells': 472928, 'visits': 474463, 'visits_short': 67093, 'streamed': 684448, 'algorithmic_bytes': 4888462, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 206346, 'bytes_per_visit_packed': 2, 'heavy_tiles': 0},
        'cells': 472928, 'off_last': 472928, 'crc': 932381198,
        'log1': ['k_profile_half<64,ss=0,pre=2,w=1,res=0> acc=0'],
        'log2': ['k_profile_half<64,ss=0,pre=2,w=1,res=1> acc=0']},
    'half_ss1': {
        'stats': {'n_ranges': 490, 'n_items': 740, 'cells': 945856, 'visits': 554105, 'visits_short': 80087, 'streamed': 847904, 'algorithmic_bytes': 7405874, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 227922, 'bytes_per_visit_packed': 2, 'heavy_tiles': 0},
        'cells': 945856, 'off_last': 945856, 'crc': 2101824091,
        'log1': ['k_profile_half<64,ss=1,pre=2,w=1,res=0> acc=0'],
        'log2': ['k_profile_half<64,ss=1,pre=2,w=1,res=1> acc=0']},
    'word_ss0': {
        'stats': {'n_ranges': 490, 'n_items': 522, 'cells': 472928, 'visits': 490932, 'visits_short': 68715, 'streamed': 698804, 'algorithmic_bytes': 5779204, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 220802, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 472928, 'off_last': 472928, 'crc': 1356011334,
        'log1': ['k_profile<64,ss=0,pre=2,w=1,res=0> acc=0'],
        'log2': ['k_profile<64,ss=0,pre=2,w=1,res=1> acc=0']},
    'word_ss1': {
        'stats': {'n_ranges': 490, 'n_items': 740, 'cells': 945856, 'visits': 585622, 'visits_short': 83649, 'streamed': 898692, 'algorithmic_bytes': 8488124, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 255181, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 945856, 'off_last': 945856, 'crc': 3279943104,
        'log1': ['k_profile<64,ss=1,pre=2,w=1,res=0> acc=0'],
        'log2': ['k_profile<64,ss=1,pre=2,w=1,res=1> acc=0']},
    'small_ss0': {
        'stats': {'n_ranges': 490, 'n_items': 474, 'cells': 67778, 'visits': 440250, 'visits_short': 62408, 'streamed': 624820, 'algorithmic_bytes': 3712728, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 203235, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 67778, 'off_last': 67778, 'crc': 2568921384,
        'log1': ['k_profile<64,ss=0,pre=2,w=1,res=0> acc=0'],
        'log2': ['k_profile_multi<ss=0,pre=2,w=8,T=4> acc=0']},
    'small_ss1': {
        'stats': {'n_ranges': 490, 'n_items': 474, 'cells': 135556, 'visits': 440250, 'visits_short': 62408, 'streamed': 624820, 'algorithmic_bytes': 3983840, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 203235, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 135556, 'off_last': 135556, 'crc': 1531418915,
        'log1': ['k_profile<64,ss=1,pre=2,w=1,res=0> acc=0'],
        'log2': ['k_profile<64,ss=1,pre=2,w=8,res=1> acc=0']},
    'count': {
        'stats': {'n_ranges': 490, 'n_items': 474, 'cells': 980, 'visits': 440250, 'visits_short': 62408, 'streamed': 624820, 'algorithmic_bytes': 3445536, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 203235, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 980, 'off_last': 980, 'crc': 2637587028,
        'log1': ['k_count_multi<T=4,pre=2> acc=0'],
        'log2': ['k_count_multi<T=4,pre=2> acc=0']},
    'cover': {
        'stats': {'n_ranges': 490, 'n_items': 522, 'cells': 472928, 'visits': 474463, 'visits_short': 67093, 'streamed': 684448, 'algorithmic_bytes': 5703712, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 206346, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 472928, 'off_last': 472928, 'crc': 4215512452,
        'log1': ['k_coverage<64,pre=2,res=0> acc=0'],
        'log2': ['k_coverage<64,pre=2,res=1> acc=0']},
    'bins2_ss0': {
        'stats': {'n_ranges': 490, 'n_items': 490, 'cells': 236576, 'visits': 451772, 'visits_short': 63974, 'streamed': 644580, 'algorithmic_bytes': 4512552, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 204300, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 236576, 'off_last': 236576, 'crc': 568629861,
        'log1': ['k_coverage_bins<64,pre=2,res=0,ss=0> acc=0 cov_reps=1'],
        'log2': ['k_coverage_bins<64,pre=2,res=1,ss=0> acc=0 cov_reps=1']},
    'bins2_ss1': {
        'stats': {'n_ranges': 490, 'n_items': 522, 'cells': 473152, 'visits': 474463, 'visits_short': 67093, 'streamed': 684448, 'algorithmic_bytes': 5704608, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 206346, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 473152, 'off_last': 473152, 'crc': 1800489448,
        'log1': ['k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=1'],
        'log2': ['k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=1']},
    'bins274_ss1': {
        'stats': {'n_ranges': 490, 'n_items': 474, 'cells': 4032, 'visits': 440250, 'visits_short': 62408, 'streamed': 624820, 'algorithmic_bytes': 3457744, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 203235, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 4032, 'off_last': 4032, 'crc': 308530933,
        'log1': ['k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=16'],
        'log2': ['k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=16']},
    'sum_half_ss0': {
        'stats': {'n_ranges': 198, 'n_items': 198, 'cells': 2048, 'visits': 239835, 'visits_short': 33896, 'streamed': 272484, 'algorithmic_bytes': 886450, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 168325, 'bytes_per_visit_packed': 2, 'heavy_tiles': 0},
        'cells': 2048, 'off_last': 405504, 'crc': 2194098404,
        'log1': ['k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=0>'],
        'log2': ['k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=1>']},
    'sum_half_ss1': {
        'stats': {'n_ranges': 198, 'n_items': 396, 'cells': 4096, 'visits': 305378, 'visits_short': 44984, 'streamed': 411156, 'algorithmic_bytes': 1389026, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 188695, 'bytes_per_visit_packed': 2, 'heavy_tiles': 0},
        'cells': 4096, 'off_last': 811008, 'crc': 3071305044,
        'log1': ['k_sum_tiles<nw=4,kSumProfile,ss=1,half=1,res=0>'],
        'log2': ['k_sum_tiles<nw=4,kSumProfile,ss=1,half=1,res=1>']},
    'sum_word_ss0': {
        'stats': {'n_ranges': 198, 'n_items': 198, 'cells': 2048, 'visits': 242402, 'visits_short': 34189, 'streamed': 274864, 'algorithmic_bytes': 1438268, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 170555, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 2048, 'off_last': 405504, 'crc': 2028385927,
        'log1': ['k_sum_tiles<nw=4,kSumProfile,ss=0,half=0,res=0>'],
        'log2': ['k_sum_tiles<nw=4,kSumProfile,ss=0,half=0,res=1>']},
    'sum_word_ss1': {
        'stats': {'n_ranges': 198, 'n_items': 396, 'cells': 4096, 'visits': 322011, 'visits_short': 47098, 'streamed': 449564, 'algorithmic_bytes': 2113924, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 202887, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 4096, 'off_last': 811008, 'crc': 1005408259,
        'log1': ['k_sum_tiles<nw=4,kSumProfile,ss=1,half=0,res=0>'],
        'log2': ['k_sum_tiles<nw=4,kSumProfile,ss=1,half=0,res=1>']},
    'sum_cover': {
        'stats': {'n_ranges': 198, 'n_items': 198, 'cells': 2048, 'visits': 239835, 'visits_short': 33896, 'streamed': 272484, 'algorithmic_bytes': 1426476, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 168325, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 2048, 'off_last': 405504, 'crc': 4114054014,
        'log1': ['k_sum_tiles<nw=4,kSumCover,ss=0,half=0,res=0>'],
        'log2': ['k_sum_tiles<nw=4,kSumCover,ss=0,half=0,res=1>']},
    'sum_cover_ss': {
        'stats': {'n_ranges': 198, 'n_items': 396, 'cells': 4096, 'visits': 305378, 'visits_short': 44984, 'streamed': 411156, 'algorithmic_bytes': 2036320, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 188695, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 4096, 'off_last': 811008, 'crc': 2163910915,
        'log1': ['k_sum_tiles<nw=4,kSumCoverSS,ss=1,half=0,res=0>'],
        'log2': ['k_sum_tiles<nw=4,kSumCoverSS,ss=1,half=0,res=1>']},
    'xcorr': {
        'stats': {'n_ranges': 490, 'n_items': 2096, 'cells': 206, 'visits': 1202955, 'visits_short': 180907, 'streamed': 2016096, 'algorithmic_bytes': 7995910, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 478304, 'bytes_per_visit_packed': 2, 'heavy_tiles': 0},
        'cells': 206, 'off_last': 945856, 'crc': 1061702822,
        'log1': ['k_xcorr_tiles<256,half=1,wide=0>'],
        'log2': ['k_xcorr_tiles<256,half=1,wide=0>']},
    'frag': {
        'stats': {'n_ranges': 490, 'n_items': 474, 'cells': 58, 'visits': 440250, 'visits_short': 62408, 'streamed': 624820, 'algorithmic_bytes': 5203080, 'bytes_per_visit_short': 12, 'bytes_per_visit_long': 16, 'visits_packed': 203235, 'bytes_per_visit_packed': 8, 'heavy_tiles': 0},
        'cells': 58, 'off_last': 490, 'runs': 474, 'crc': 3377928048,
        'log1': ['k_frag_tiles<256,merge=0,ltab=1>'],
        'log2': ['k_frag_tiles<256,merge=0,ltab=1>']},
    'hist': {
        'stats': {'n_ranges': 490, 'n_items': 2096, 'cells': 53, 'visits': 1064177, 'visits_short': 162226, 'streamed': 1882004, 'algorithmic_bytes': 7680510, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 361869, 'bytes_per_visit_packed': 2, 'heavy_tiles': 0},
        'cells': 53, 'off_last': 945856, 'runs': 1048, 'crc': 3439107365,
        'log1': ['k_hist_tiles<256,kHistEndsHalf,wide=0,form=0>'],
        'log2': ['k_hist_tiles<256,kHistEndsHalf,wide=0,form=0>']},
    'summary': {
        'stats': {'n_ranges': 490, 'n_items': 23926, 'cells': 5390, 'visits': 9236332, 'visits_short': 1483080, 'streamed': 19942900, 'algorithmic_bytes': 87465376, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 2400510, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 5390, 'off_last': 472928, 'runs': 1260, 'crc': 767324372,
        'log1': ['k_summary_tiles<256,kHistCover,wide=0>'],
        'log2': ['k_summary_tiles<256,kHistCover,wide=0>']},
    'scaled': {
        'stats': {'n_ranges': 490, 'n_items': 522, 'cells': 19600, 'visits': 474463, 'visits_short': 67093, 'streamed': 684448, 'algorithmic_bytes': 3153550, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 206346, 'bytes_per_visit_packed': 2, 'heavy_tiles': 0},
        'cells': 19600, 'off_last': 945856, 'runs': 522, 'crc': 2377955766,
        'log1': ['k_scaled_tiles<256,kHistEndsHalf,wide=0,seg=0>'],
        'log2': ['k_scaled_tiles<256,kHistEndsHalf,wide=0,seg=0>']},
    'resized': {
        'stats': {'n_ranges': 490, 'n_items': 522, 'cells': 472928, 'visits': 507140, 'visits_short': 70367, 'streamed': 712160, 'algorithmic_bytes': 5854028, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 234935, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 472928, 'off_last': 472928, 'crc': 2359379893,
        'log1': ['k_coverage<64,pre=2,res=0,frag=1> acc=0'],
        'log2': ['k_coverage<64,pre=2,res=1,frag=1> acc=0']},
    'overlap_tile': {
        'stats': {'n_ranges': 490, 'n_items': 5026, 'cells': 980, 'visits': 2145656, 'visits_short': 338562, 'streamed': 4309912, 'algorithmic_bytes': 19663888, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 636941, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 980, 'off_last': 980, 'crc': 1790891161,
        'log1': ['k_overlap_multi<T=4,pre=2,within=0> acc=0'],
        'log2': ['k_overlap_multi<T=4,pre=2,within=0> acc=0']},
    'wide_bins': {
        'stats': {'n_ranges': 493, 'n_items': 487, 'cells': 974, 'visits': 474246, 'visits_short': 66327, 'streamed': 667068, 'algorithmic_bytes': 3630892, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 229214, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 974, 'off_last': 974, 'crc': 1401480375,
        'log1': ['k_count_multi<T=4,pre=2> acc=0'],
        'log2': ['k_count_multi<T=4,pre=2> acc=0']},
    'count_long': {
        'stats': {'n_ranges': 1, 'n_items': 3, 'cells': 2, 'visits': 12393, 'visits_short': 1308, 'streamed': 14344, 'algorithmic_bytes': 64972, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 9842, 'bytes_per_visit_packed': 4, 'heavy_tiles': 0},
        'cells': 2, 'off_last': 2, 'crc': 636000472,
        'log1': ['k_count_multi<T=4,pre=2> acc=0'],
        'log2': ['k_count_multi<T=4,pre=2> acc=0']},
    'heavy_half_ss1': {
        'stats': {'n_ranges': 490, 'n_items': 740, 'cells': 945856, 'visits': 554105, 'visits_short': 80087, 'streamed': 847904, 'algorithmic_bytes': 7405874, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 227922, 'bytes_per_visit_packed': 2, 'heavy_tiles': 649},
        'cells': 945856, 'off_last': 945856, 'crc': 2101824091,
        'log1': ['k_profile_half<64,ss=1,pre=2,w=1,res=0> acc=0', 'k_profile_half<64,ss=1,pre=2,w=1,res=0> acc=1'],
        'log2': ['k_profile_half<64,ss=1,pre=2,w=1,res=1> acc=0', 'k_profile_half<64,ss=1,pre=2,w=1,res=0> acc=1']},
    'heavy_bins2_ss1': {
        'stats': {'n_ranges': 490, 'n_items': 522, 'cells': 473152, 'visits': 474463, 'visits_short': 67093, 'streamed': 684448, 'algorithmic_bytes': 5704608, 'bytes_per_visit_short': 8, 'bytes_per_visit_long': 12, 'visits_packed': 206346, 'bytes_per_visit_packed': 4, 'heavy_tiles': 480},
        'cells': 473152, 'off_last': 473152, 'crc': 1800489448,
        'log1': ['k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=1', 'k_coverage_bins<64,pre=2,res=0,ss=1> acc=1 cov_reps=1'],
        'log2': ['k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=1', 'k_coverage_bins<64,pre=2,res=0,ss=1> acc=1 cov_reps=1']},
    'heavy_sum_half_ss0': {
        'stats': {'n_ranges': 198, 'n_items': 198, 'cells': 2048, 'visits': 239835, 'visits_short': 33896, 'streamed': 272484, 'algorithmic_bytes': 886450, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 168325, 'bytes_per_visit_packed': 2, 'heavy_tiles': 156},
        'cells': 2048, 'off_last': 405504, 'crc': 2194098404,
        'log1': ['k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=0>', 'k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=0>'],
        'log2': ['k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=1>', 'k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=0>']},
    'heavy_hist': {
        'stats': {'n_ranges': 490, 'n_items': 2096, 'cells': 53, 'visits': 1064177, 'visits_short': 162226, 'streamed': 1882004, 'algorithmic_bytes': 7680510, 'bytes_per_visit_short': 2, 'bytes_per_visit_long': 12, 'visits_packed': 361869, 'bytes_per_visit_packed': 2, 'heavy_tiles': 1695},
        'cells': 53, 'off_last': 945856, 'runs': 2743, 'crc': 3439107365,
        'log1': ['k_hist_tiles<256,kHistEndsHalf,wide=0,form=0>', 'k_hist_tiles<256,kHistEnds,wide=1,form=0>'],
        'log2': ['k_hist_tiles<256,kHistEndsHalf,wide=0,form=0>', 'k_hist_tiles<256,kHistEnds,wide=1,form=0>']},
}


def test_the_table_names_every_case():
    assert list(EXPECTED) == CASES and len(set(CASES)) == len(CASES)
    heavy = [n for n in CASES if n.startswith("heavy_")]
    assert len(heavy) == 4 and all(EXPECTED[n]["stats"]["heavy_tiles"] > 0 for n in heavy)
    assert EXPECTED["heavy_bins2_ss1"]["stats"]["heavy_tiles"] and not EXPECTED["bins2_ss1"]["stats"]["heavy_tiles"]
    # the wide cases are what they are for: 40,000 bases are three tiles of a bamCount, five bins of 8,193 (and 20,000 three)
    assert EXPECTED["count_long"]["stats"]["n_items"] == 3
    assert EXPECTED["wide_bins"]["stats"]["n_items"] == EXPECTED["count"]["stats"]["n_items"] + 5 + 5 + 3
    assert EXPECTED["wide_bins"]["log1"][0].startswith("k_count")


@pytest.mark.parametrize("name", CASES)
def test_plan_is_the_recorded_one(gpu, name):
    got = record(*gpu, name)
    want = EXPECTED[name]
    assert got["stats"] == want["stats"], {k: (v, want["stats"][k]) for k, v in got["stats"].items() if v != want["stats"][k]}
    assert got == want


if __name__ == "__main__":
    with _resident() as g:
        print("EXPECTED = ", end="")
        pprint.pprint({name: record(*g, name) for name in CASES}, width=150, sort_dicts=False)
