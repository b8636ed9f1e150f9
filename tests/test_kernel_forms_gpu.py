"""GPU: every pileup and sum-tiles kernel form that launch_mode and sum_form (csrc/kernels.hip) can launch, run
on tests/forms_deck.py's reads and ranges and compared with the C oracle cell by cell, exactly.  A case sets the tuning
knobs (bsig_debug_set_knob) and call parameters that select one form, turns the launch log on (bsig_debug_launch_log),
makes a plan, runs it twice -- the first run looks its windows up in the kernel, the second takes the form for resolved
windows; the 8-wave and multi-tile forms, which exist for resolved windows only, resolve from the first run on -- and
asserts that the log holds exactly the forms the case names.  The last test holds the list of all form names and
compares it with what the cases saw: a form nobody reached fails it, and so does a form nobody listed.

Knobs: 0 k_profile's class-0 passes in flight, 1 / 2 the count family's tiles per wave and passes, 3 the 8-wave build
(8 always, 1 never), 4 resolve from n tiles on, 5 tiles per wave of the profile forms (1, 2, 4), 6 the half form's passes.
The half form (k_profile_half, k_profile_multi_half) needs the packed class's 16-bit column: the layout without a packed
class (BAMSIGNALS_PACK=0) runs the 4-byte forms only, for which it is the one that fills class 0's windows.  On the
default layout a half form also reads span classes 0 and 1 from their 16-bit columns (bytes_per_visit_short 2), class 0
through the deck's class-0 islands; the layout made under BAMSIGNALS_SHORT_HALF=0 keeps those two classes on pos + fm (8)
under the same half forms."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import forms_deck as deck

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {0: 2, 1: 0, 2: 0, 3: 0, 5: 0, 6: 2}
SEEN = set()            # every form name a case of this module logged (test_every_form_was_reached reads it)
LAYOUTS = ("packed", "nopack")

ALL_FORMS = (
    "k_profile<64,ss=0,pre=2,w=1,res=0> acc=0",
    "k_profile<64,ss=0,pre=2,w=1,res=1> acc=0",
    "k_profile<64,ss=0,pre=2,w=1,res=0> acc=1",
    "k_profile<64,ss=0,pre=3,w=1,res=0> acc=0",
    "k_profile<64,ss=0,pre=3,w=1,res=1> acc=0",
    "k_profile<64,ss=0,pre=3,w=1,res=0> acc=1",
    "k_profile<64,ss=0,pre=4,w=1,res=0> acc=0",
    "k_profile<64,ss=0,pre=4,w=1,res=1> acc=0",
    "k_profile<64,ss=0,pre=4,w=1,res=0> acc=1",
    "k_profile<64,ss=1,pre=2,w=1,res=0> acc=0",
    "k_profile<64,ss=1,pre=2,w=1,res=1> acc=0",
    "k_profile<64,ss=1,pre=2,w=1,res=0> acc=1",
    "k_profile<64,ss=1,pre=3,w=1,res=0> acc=0",
    "k_profile<64,ss=1,pre=3,w=1,res=1> acc=0",
    "k_profile<64,ss=1,pre=3,w=1,res=0> acc=1",
    "k_profile<64,ss=1,pre=4,w=1,res=0> acc=0",
    "k_profile<64,ss=1,pre=4,w=1,res=1> acc=0",
    "k_profile<64,ss=1,pre=4,w=1,res=0> acc=1",
    "k_profile<128,ss=0,pre=2,w=1,res=0> acc=0",
    "k_profile<128,ss=0,pre=2,w=1,res=1> acc=0",
    "k_profile<128,ss=0,pre=2,w=1,res=0> acc=1",
    "k_profile<128,ss=0,pre=3,w=1,res=0> acc=0",
    "k_profile<128,ss=0,pre=3,w=1,res=1> acc=0",
    "k_profile<128,ss=0,pre=3,w=1,res=0> acc=1",
    "k_profile<128,ss=0,pre=4,w=1,res=0> acc=0",
    "k_profile<128,ss=0,pre=4,w=1,res=1> acc=0",
    "k_profile<128,ss=0,pre=4,w=1,res=0> acc=1",
    "k_profile<128,ss=1,pre=2,w=1,res=0> acc=0",
    "k_profile<128,ss=1,pre=2,w=1,res=1> acc=0",
    "k_profile<128,ss=1,pre=2,w=1,res=0> acc=1",
    "k_profile<128,ss=1,pre=3,w=1,res=0> acc=0",
    "k_profile<128,ss=1,pre=3,w=1,res=1> acc=0",
    "k_profile<128,ss=1,pre=3,w=1,res=0> acc=1",
    "k_profile<128,ss=1,pre=4,w=1,res=0> acc=0",
    "k_profile<128,ss=1,pre=4,w=1,res=1> acc=0",
    "k_profile<128,ss=1,pre=4,w=1,res=0> acc=1",
    "k_profile<256,ss=0,pre=2,w=1,res=0> acc=0",
    "k_profile<256,ss=0,pre=2,w=1,res=1> acc=0",
    "k_profile<256,ss=0,pre=2,w=1,res=0> acc=1",
    "k_profile<256,ss=0,pre=3,w=1,res=0> acc=0",
    "k_profile<256,ss=0,pre=3,w=1,res=1> acc=0",
    "k_profile<256,ss=0,pre=3,w=1,res=0> acc=1",
    "k_profile<256,ss=0,pre=4,w=1,res=0> acc=0",
    "k_profile<256,ss=0,pre=4,w=1,res=1> acc=0",
    "k_profile<256,ss=0,pre=4,w=1,res=0> acc=1",
    "k_profile<256,ss=1,pre=2,w=1,res=0> acc=0",
    "k_profile<256,ss=1,pre=2,w=1,res=1> acc=0",
    "k_profile<256,ss=1,pre=2,w=1,res=0> acc=1",
    "k_profile<256,ss=1,pre=3,w=1,res=0> acc=0",
    "k_profile<256,ss=1,pre=3,w=1,res=1> acc=0",
    "k_profile<256,ss=1,pre=3,w=1,res=0> acc=1",
    "k_profile<256,ss=1,pre=4,w=1,res=0> acc=0",
    "k_profile<256,ss=1,pre=4,w=1,res=1> acc=0",
    "k_profile<256,ss=1,pre=4,w=1,res=0> acc=1",
    "k_profile<64,ss=0,pre=2,w=8,res=1> acc=0",
    "k_profile<64,ss=1,pre=2,w=8,res=1> acc=0",
    "k_profile_half<64,ss=0,pre=1,w=1,res=0> acc=0",
    "k_profile_half<64,ss=0,pre=1,w=1,res=1> acc=0",
    "k_profile_half<64,ss=0,pre=1,w=1,res=0> acc=1",
    "k_profile_half<64,ss=0,pre=2,w=1,res=0> acc=0",
    "k_profile_half<64,ss=0,pre=2,w=1,res=1> acc=0",
    "k_profile_half<64,ss=0,pre=2,w=1,res=0> acc=1",
    "k_profile_half<64,ss=1,pre=1,w=1,res=0> acc=0",
    "k_profile_half<64,ss=1,pre=1,w=1,res=1> acc=0",
    "k_profile_half<64,ss=1,pre=1,w=1,res=0> acc=1",
    "k_profile_half<64,ss=1,pre=2,w=1,res=0> acc=0",
    "k_profile_half<64,ss=1,pre=2,w=1,res=1> acc=0",
    "k_profile_half<64,ss=1,pre=2,w=1,res=0> acc=1",
    "k_profile_half<128,ss=0,pre=1,w=1,res=0> acc=0",
    "k_profile_half<128,ss=0,pre=1,w=1,res=1> acc=0",
    "k_profile_half<128,ss=0,pre=1,w=1,res=0> acc=1",
    "k_profile_half<128,ss=0,pre=2,w=1,res=0> acc=0",
    "k_profile_half<128,ss=0,pre=2,w=1,res=1> acc=0",
    "k_profile_half<128,ss=0,pre=2,w=1,res=0> acc=1",
    "k_profile_half<128,ss=1,pre=1,w=1,res=0> acc=0",
    "k_profile_half<128,ss=1,pre=1,w=1,res=1> acc=0",
    "k_profile_half<128,ss=1,pre=1,w=1,res=0> acc=1",
    "k_profile_half<128,ss=1,pre=2,w=1,res=0> acc=0",
    "k_profile_half<128,ss=1,pre=2,w=1,res=1> acc=0",
    "k_profile_half<128,ss=1,pre=2,w=1,res=0> acc=1",
    "k_profile_half<256,ss=0,pre=1,w=1,res=0> acc=0",
    "k_profile_half<256,ss=0,pre=1,w=1,res=1> acc=0",
    "k_profile_half<256,ss=0,pre=1,w=1,res=0> acc=1",
    "k_profile_half<256,ss=0,pre=2,w=1,res=0> acc=0",
    "k_profile_half<256,ss=0,pre=2,w=1,res=1> acc=0",
    "k_profile_half<256,ss=0,pre=2,w=1,res=0> acc=1",
    "k_profile_half<256,ss=1,pre=1,w=1,res=0> acc=0",
    "k_profile_half<256,ss=1,pre=1,w=1,res=1> acc=0",
    "k_profile_half<256,ss=1,pre=1,w=1,res=0> acc=1",
    "k_profile_half<256,ss=1,pre=2,w=1,res=0> acc=0",
    "k_profile_half<256,ss=1,pre=2,w=1,res=1> acc=0",
    "k_profile_half<256,ss=1,pre=2,w=1,res=0> acc=1",
    "k_profile_half<64,ss=0,pre=1,w=8,res=1> acc=0",
    "k_profile_half<64,ss=0,pre=2,w=8,res=1> acc=0",
    "k_profile_half<64,ss=1,pre=1,w=8,res=1> acc=0",
    "k_profile_half<64,ss=1,pre=2,w=8,res=1> acc=0",
    "k_profile_multi<ss=0,pre=2,w=1,T=2> acc=0",
    "k_profile_multi<ss=0,pre=2,w=1,T=4> acc=0",
    "k_profile_multi<ss=0,pre=2,w=8,T=2> acc=0",
    "k_profile_multi<ss=0,pre=2,w=8,T=4> acc=0",
    "k_profile_multi<ss=1,pre=2,w=1,T=2> acc=0",
    "k_profile_multi<ss=1,pre=2,w=1,T=4> acc=0",
    "k_profile_multi<ss=1,pre=2,w=8,T=2> acc=0",
    "k_profile_multi<ss=1,pre=2,w=8,T=4> acc=0",
    "k_profile_multi_half<ss=0,pre=1,w=1,T=2> acc=0",
    "k_profile_multi_half<ss=0,pre=1,w=1,T=4> acc=0",
    "k_profile_multi_half<ss=0,pre=1,w=8,T=2> acc=0",
    "k_profile_multi_half<ss=0,pre=1,w=8,T=4> acc=0",
    "k_profile_multi_half<ss=0,pre=2,w=1,T=2> acc=0",
    "k_profile_multi_half<ss=0,pre=2,w=1,T=4> acc=0",
    "k_profile_multi_half<ss=0,pre=2,w=8,T=2> acc=0",
    "k_profile_multi_half<ss=0,pre=2,w=8,T=4> acc=0",
    "k_profile_multi_half<ss=1,pre=1,w=1,T=2> acc=0",
    "k_profile_multi_half<ss=1,pre=1,w=1,T=4> acc=0",
    "k_profile_multi_half<ss=1,pre=1,w=8,T=2> acc=0",
    "k_profile_multi_half<ss=1,pre=1,w=8,T=4> acc=0",
    "k_profile_multi_half<ss=1,pre=2,w=1,T=2> acc=0",
    "k_profile_multi_half<ss=1,pre=2,w=1,T=4> acc=0",
    "k_profile_multi_half<ss=1,pre=2,w=8,T=2> acc=0",
    "k_profile_multi_half<ss=1,pre=2,w=8,T=4> acc=0",
    "k_profile_small<64,ss=0,res=0> acc=0",
    "k_profile_small<64,ss=0,res=1> acc=0",
    "k_profile_small<64,ss=0,res=0> acc=1",
    "k_profile_small<64,ss=1,res=0> acc=0",
    "k_profile_small<64,ss=1,res=1> acc=0",
    "k_profile_small<64,ss=1,res=0> acc=1",
    "k_profile_small<128,ss=0,res=0> acc=0",
    "k_profile_small<128,ss=0,res=1> acc=0",
    "k_profile_small<128,ss=0,res=0> acc=1",
    "k_profile_small<128,ss=1,res=0> acc=0",
    "k_profile_small<128,ss=1,res=1> acc=0",
    "k_profile_small<128,ss=1,res=0> acc=1",
    "k_profile_small<256,ss=0,res=0> acc=0",
    "k_profile_small<256,ss=0,res=1> acc=0",
    "k_profile_small<256,ss=0,res=0> acc=1",
    "k_profile_small<256,ss=1,res=0> acc=0",
    "k_profile_small<256,ss=1,res=1> acc=0",
    "k_profile_small<256,ss=1,res=0> acc=1",
    "k_coverage<64,pre=2,res=0> acc=0",
    "k_coverage<64,pre=2,res=1> acc=0",
    "k_coverage<64,pre=2,res=0> acc=1",
    "k_coverage<128,pre=2,res=0> acc=0",
    "k_coverage<128,pre=2,res=1> acc=0",
    "k_coverage<128,pre=2,res=0> acc=1",
    "k_coverage<256,pre=2,res=0> acc=0",
    "k_coverage<256,pre=2,res=1> acc=0",
    "k_coverage<256,pre=2,res=0> acc=1",
    "k_coverage_bins<64,pre=2,res=0,ss=0> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=1,ss=0> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=0,ss=0> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=1,ss=0> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=0,ss=0> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=1,ss=0> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=0,ss=0> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=1,ss=0> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=0,ss=0> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=1,ss=0> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=0,ss=0> acc=1 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=16",
    "k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=8",
    "k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=4",
    "k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=2",
    "k_coverage_bins<64,pre=2,res=0,ss=1> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=1,ss=1> acc=0 cov_reps=1",
    "k_coverage_bins<64,pre=2,res=0,ss=1> acc=1 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=0> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=1,ss=0> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=0> acc=1 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=1> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=1,ss=1> acc=0 cov_reps=8",
    "k_coverage_bins<128,pre=2,res=0,ss=1> acc=1 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=0> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=1,ss=0> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=0> acc=1 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=1> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=1,ss=1> acc=0 cov_reps=8",
    "k_coverage_bins<256,pre=2,res=0,ss=1> acc=1 cov_reps=8",
    "k_count<64> acc=0",
    "k_count<64> acc=1",
    "k_count<128> acc=0",
    "k_count<128> acc=1",
    "k_count<256> acc=0",
    "k_count<256> acc=1",
    "k_count_multi<T=2,pre=2> acc=0",
    "k_count_multi<T=2,pre=3> acc=0",
    "k_count_multi<T=2,pre=4> acc=0",
    "k_count_multi<T=4,pre=2> acc=0",
    "k_count_multi<T=4,pre=3> acc=0",
    "k_count_multi<T=4,pre=4> acc=0",
    "k_count_multi<T=8,pre=2> acc=0",
    "k_count_multi<T=8,pre=3> acc=0",
    "k_count_multi<T=8,pre=4> acc=0",
    "k_sum_tiles<nw=1,kSumProfile,ss=0,half=0,res=0>",
    "k_sum_tiles<nw=1,kSumProfile,ss=0,half=0,res=1>",
    "k_sum_tiles<nw=1,kSumProfile,ss=0,half=1,res=0>",
    "k_sum_tiles<nw=1,kSumProfile,ss=0,half=1,res=1>",
    "k_sum_tiles<nw=1,kSumProfile,ss=1,half=0,res=0>",
    "k_sum_tiles<nw=1,kSumProfile,ss=1,half=0,res=1>",
    "k_sum_tiles<nw=1,kSumProfile,ss=1,half=1,res=0>",
    "k_sum_tiles<nw=1,kSumProfile,ss=1,half=1,res=1>",
    "k_sum_tiles<nw=1,kSumCover,ss=0,half=0,res=0>",
    "k_sum_tiles<nw=1,kSumCover,ss=0,half=0,res=1>",
    "k_sum_tiles<nw=1,kSumCoverSS,ss=1,half=0,res=0>",
    "k_sum_tiles<nw=1,kSumCoverSS,ss=1,half=0,res=1>",
    "k_sum_tiles<nw=2,kSumProfile,ss=0,half=0,res=0>",
    "k_sum_tiles<nw=2,kSumProfile,ss=0,half=0,res=1>",
    "k_sum_tiles<nw=2,kSumProfile,ss=0,half=1,res=0>",
    "k_sum_tiles<nw=2,kSumProfile,ss=0,half=1,res=1>",
    "k_sum_tiles<nw=2,kSumProfile,ss=1,half=0,res=0>",
    "k_sum_tiles<nw=2,kSumProfile,ss=1,half=0,res=1>",
    "k_sum_tiles<nw=2,kSumProfile,ss=1,half=1,res=0>",
    "k_sum_tiles<nw=2,kSumProfile,ss=1,half=1,res=1>",
    "k_sum_tiles<nw=2,kSumCover,ss=0,half=0,res=0>",
    "k_sum_tiles<nw=2,kSumCover,ss=0,half=0,res=1>",
    "k_sum_tiles<nw=2,kSumCoverSS,ss=1,half=0,res=0>",
    "k_sum_tiles<nw=2,kSumCoverSS,ss=1,half=0,res=1>",
    "k_sum_tiles<nw=4,kSumProfile,ss=0,half=0,res=0>",
    "k_sum_tiles<nw=4,kSumProfile,ss=0,half=0,res=1>",
    "k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=0>",
    "k_sum_tiles<nw=4,kSumProfile,ss=0,half=1,res=1>",
    "k_sum_tiles<nw=4,kSumProfile,ss=1,half=0,res=0>",
    "k_sum_tiles<nw=4,kSumProfile,ss=1,half=0,res=1>",
    "k_sum_tiles<nw=4,kSumProfile,ss=1,half=1,res=0>",
    "k_sum_tiles<nw=4,kSumProfile,ss=1,half=1,res=1>",
    "k_sum_tiles<nw=4,kSumCover,ss=0,half=0,res=0>",
    "k_sum_tiles<nw=4,kSumCover,ss=0,half=0,res=1>",
    "k_sum_tiles<nw=4,kSumCoverSS,ss=1,half=0,res=0>",
    "k_sum_tiles<nw=4,kSumCoverSS,ss=1,half=0,res=1>",
)


# ---------------------------------------------------------------------------------------------------------------
# the reads in both layouts, the knobs, the log
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    """(context, {layout: Reads}): the deck's reads with the packed class (default), with it but without the columns of
    span classes 0 and 1 (BAMSIGNALS_SHORT_HALF=0), and without a packed class (BAMSIGNALS_PACK=0)"""
    from bamsignals_amd.device import Context, Reads
    c = deck.reads()
    ctx = Context(0)
    out = {}
    switches = {"packed": None, "packed_noshort": "BAMSIGNALS_SHORT_HALF", "nopack": "BAMSIGNALS_PACK"}
    old = {name: os.environ.get(name) for name in switches.values() if name}
    try:
        for layout, name in switches.items():
            for other in old:
                os.environ.pop(other, None)
            if name:
                os.environ[name] = "0"
            out[layout] = Reads(ctx, c["ref_len"], c["ref_off"], c["pos"], c["flag"], c["mapq"], c["tlen"], end=c["end"])
    finally:
        for name, value in old.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value
    info = {k: r.info() for k, r in out.items()}
    assert info["packed"]["class_n"][4] > 0 and info["nopack"]["class_n"][4] == 0
    assert info["packed"]["class_n"][0] > 19_000 and list(info["packed_noshort"]["class_n"]) == list(info["packed"]["class_n"])
    yield ctx, out
    for r in out.values():
        r.close()
    ctx.close()


def _lib_fns():
    from bamsignals_amd import _lib
    lib = _lib.load()
    log = lib.bsig_debug_launch_log
    log.argtypes, log.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    return lib.bsig_debug_set_knob, log


@contextlib.contextmanager
def _selected(knobs, resolved_first=False, heavy=False):
    """the knobs set, the log on and empty; yields drain() -> the names logged since; everything restored on the way out"""
    knob, log = _lib_fns()
    old_heavy = os.environ.get("BAMSIGNALS_HEAVY_READS")
    buf = ctypes.create_string_buffer(65537)

    def drain():
        n = log(buf, len(buf))
        names = buf.value.decode().splitlines()
        assert n == len(names)
        return names
    try:
        for k, v in knobs.items():
            assert knob(k, v) == 0
        if resolved_first:
            assert knob(4, 1) == 0
        if heavy:
            os.environ["BAMSIGNALS_HEAVY_READS"] = "64"
        assert log(None, 1) >= 0
        yield drain
    finally:
        log(None, 0)
        for k, v in KNOB_DEFAULTS.items():
            knob(k, v)
        knob(4, -1)
        if old_heavy is None:
            os.environ.pop("BAMSIGNALS_HEAVY_READS", None)
        else:
            os.environ["BAMSIGNALS_HEAVY_READS"] = old_heavy


def _case(gpu, layout, name, expect, knobs, tile_cells=0, threads=0, resolved_first=False, heavy=False, bpv=None, residue=None,
          count=False):
    """One case: PARAM_SETS[name] on the deck (or on its cut with `residue` tiles modulo 8), both runs against the oracle,
    the log against `expect`."""
    from bamsignals_amd.device import Plan, make_params
    ctx, reads = gpu
    mode, a = deck.gpu_args(name)
    if residue is None:
        rg, want = deck.ranges(), deck.expected(name)[0]
    else:
        rg, k = deck.cut(None if count else tile_cells, residue, a.get("binsize", 1) if not count else 1)
        want = deck.cut_expected(name, k)
    with _selected(knobs, resolved_first, heavy) as drain:
        plan = Plan(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(mode, tile_cells=tile_cells, threads=threads, **a))
        try:
            first, second, st = plan.run_host().copy(), plan.run_host().copy(), plan.stats()
        finally:
            plan.close()
        names = drain()
    SEEN.update(names)
    assert want.any()
    assert np.array_equal(first, want), (names, int(np.sum(first != want)))
    assert np.array_equal(second, want), (names, int(np.sum(second != want)))
    assert set(names) == set(expect), (names, expect)
    if bpv is not None:
        assert st["bytes_per_visit_packed"] == bpv
    if bpv == 2:                                     # a half form: classes 0 and 1 from their columns where the layout has them
        assert st["bytes_per_visit_short"] == (8 if layout == "packed_noshort" else 2), (layout, st["bytes_per_visit_short"])
        assert st["visits_short"] > 0
    if residue is not None:
        assert st["n_items"] % 8 == residue, st["n_items"]
    assert (st["heavy_tiles"] > 0) == heavy
    return st


def _kp(kernel, nt, ss, pre, w, res, acc=0):
    return f"{kernel}<{nt},ss={int(ss)},pre={pre},w={w},res={res}> acc={acc}"


def _profile_kind(layout, kind):
    """(parameter-set prefix, bytes a packed visit, the knob of its passes in flight)"""
    if kind == "half":
        assert layout in ("packed", "packed_noshort")
        return "half", 2, 6
    return "word", 4, 0


PROFILE_KINDS = [("packed", "half", p) for p in (1, 2)] + [(lay, "word", p) for lay in LAYOUTS for p in (2, 3, 4)]
PROFILE_KINDS_W8 = [("packed", "half", p) for p in (1, 2)] + [(lay, "word", 2) for lay in LAYOUTS]


def _kernel(kind, multi=False):
    return ("k_profile_multi" if multi else "k_profile") + ("_half" if kind == "half" else "")


# ---------------------------------------------------------------------------------------------------------------
# bamProfile per base: k_profile, k_profile_half and their multi-tile forms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [256, 2048])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("nt", [64, 128, 256])
@pytest.mark.parametrize("layout,kind,pre", PROFILE_KINDS + [("packed_noshort", "half", p) for p in (1, 2)])
def test_profile_one_tile_per_workgroup(gpu, layout, kind, pre, nt, ss, tile):
    """the 1-wave-budget build on narrow and wide tiles: fused, then resolved"""
    K, (pset, bpv, pre_knob) = _kernel(kind), _profile_kind(layout, kind)
    _case(gpu, layout, f"{pset}_ss{int(ss)}", [_kp(K, nt, ss, pre, 1, 0), _kp(K, nt, ss, pre, 1, 1)], {pre_knob: pre, 3: 1, 5: 1},
          tile_cells=tile, threads=nt, bpv=bpv)


@pytest.mark.parametrize("tile", [256, 2048])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("layout,kind,pre", PROFILE_KINDS_W8)
def test_profile_eight_wave_build(gpu, layout, kind, pre, ss, tile):
    """the build for 8 waves per SIMD forced on narrow and on wide tiles (resolved windows only)"""
    K, (pset, bpv, pre_knob) = _kernel(kind), _profile_kind(layout, kind)
    _case(gpu, layout, f"{pset}_ss{int(ss)}", [_kp(K, 64, ss, pre, 8, 1)], {pre_knob: pre, 3: 8, 5: 1}, tile_cells=tile, threads=64,
          resolved_first=True, bpv=bpv)


@pytest.mark.parametrize("tile,residue", [(256, 0), (256, 7), (256, 1), (2048, 7)])
@pytest.mark.parametrize("per_wave", [2, 4])
@pytest.mark.parametrize("w", [1, 8])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("layout,kind,pre", PROFILE_KINDS_W8)
def test_profile_several_tiles_per_wave(gpu, layout, kind, pre, ss, w, per_wave, tile, residue):
    """k_profile_multi / k_profile_multi_half: consecutive tiles of very different size through one LDS image, a full,
    an almost full and a one-tile last workgroup"""
    K, (pset, bpv, pre_knob) = _kernel(kind, multi=True), _profile_kind(layout, kind)
    _case(gpu, layout, f"{pset}_ss{int(ss)}", [f"{K}<ss={int(ss)},pre={pre},w={w},T={per_wave}> acc=0"],
          {pre_knob: pre, 3: w, 5: per_wave}, tile_cells=tile, threads=64, resolved_first=True, bpv=bpv, residue=residue)


def test_profile_several_tiles_per_wave_without_the_short_columns(gpu):
    """k_profile_multi_half with four tiles a wave where classes 0 and 1 come from pos + fm"""
    _case(gpu, "packed_noshort", "half_ss1", ["k_profile_multi_half<ss=1,pre=2,w=1,T=4> acc=0"], {6: 2, 3: 1, 5: 4}, tile_cells=256,
          threads=64, resolved_first=True, bpv=2, residue=7)


@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("nt", [64, 128, 256])
@pytest.mark.parametrize("layout,kind,pre", PROFILE_KINDS)
def test_profile_heavy_tiles_accumulate(gpu, layout, kind, pre, nt, ss):
    """tiles of more than 64 reads cut into slices that a second launch of the same kernel adds up (accumulate = 1)"""
    K, (pset, bpv, pre_knob) = _kernel(kind), _profile_kind(layout, kind)
    _case(gpu, layout, f"{pset}_ss{int(ss)}", [_kp(K, nt, ss, pre, 1, 0), _kp(K, nt, ss, pre, 1, 1), _kp(K, nt, ss, pre, 1, 0, acc=1)],
          {pre_knob: pre, 3: 1, 5: 1}, tile_cells=256, threads=nt, heavy=True, bpv=bpv)


# ---------------------------------------------------------------------------------------------------------------
# bamProfile with bins in a small image: k_profile_small
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("nt", [64, 128, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_profile_small(gpu, layout, nt, ss, heavy):
    form = f"k_profile_small<{nt},ss={int(ss)},res=%d> acc=%d"
    _case(gpu, layout, f"small_ss{int(ss)}", [form % (0, 0), form % (1, 0)] + ([form % (0, 1)] if heavy else []), {},
          tile_cells=64, threads=nt, heavy=heavy)


# ---------------------------------------------------------------------------------------------------------------
# bamCoverage: k_coverage, k_coverage_bins
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,heavy", [(256, False), (2048, False), (256, True)])
@pytest.mark.parametrize("nt", [64, 128, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_coverage(gpu, layout, nt, tile, heavy):
    form = f"k_coverage<{nt},pre=2,res=%d> acc=%d"
    _case(gpu, layout, "cover", [form % (0, 0), form % (1, 0)] + ([form % (0, 1)] if heavy else []), {}, tile_cells=tile,
          threads=nt, heavy=heavy)


def cov_reps(cells):
    """the replicas of k_coverage_bins' image by its values per tile: as many copies as fit 8 KiB, at most 16
    (16-B vectors of one copy: ((cells + 7) / 4) | 1)"""
    vec = ((cells + 7) // 4) | 1
    r = 1
    while r < 16 and 2 * r * vec * 16 <= 8192:
        r *= 2
    return r


# (parameter set, tile_cells, values per tile, replicas): both sides of every change of the replica count
COV_BINS = [("bins2_ss0", t, t, r) for t, r in ((120, 16), (124, 8), (248, 8), (252, 4), (504, 4), (508, 2), (1016, 2), (1020, 1))] + \
           [("bins2_ss1", t, 2 * t, r) for t, r in ((64, 8), (124, 8), (128, 4), (252, 4), (256, 2), (508, 2), (512, 1))] + \
           [("bins274_ss1", 0, 120, 16)]      # (60-cell tiles by the library's own rule for 274-bp bins: 16,384 / 274)


def test_cov_reps_table():
    for _, _, cells, r in COV_BINS:
        assert cov_reps(cells) == r, cells
    for ss in ("ss0", "ss1"):
        assert {r for pset, _, _, r in COV_BINS if pset.endswith(ss)} == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("pset,tile,cells,reps", COV_BINS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_coverage_bins_replicas(gpu, layout, pset, tile, cells, reps):
    ss = int(pset.endswith("ss1"))
    form = f"k_coverage_bins<64,pre=2,res=%d,ss={ss}> acc=0 cov_reps={reps}"
    _case(gpu, layout, pset, [form % 0, form % 1], {}, tile_cells=tile, threads=64)


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("nt", [64, 128, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_coverage_bins_workgroups(gpu, layout, nt, ss, heavy):
    form = f"k_coverage_bins<{nt},pre=2,res=%d,ss={int(ss)}> acc=%d cov_reps=8"
    _case(gpu, layout, f"bins2_ss{int(ss)}", [form % (0, 0), form % (1, 0)] + ([form % (0, 1)] if heavy else []), {},
          tile_cells=64 if ss else 124, threads=nt, heavy=heavy)


# ---------------------------------------------------------------------------------------------------------------
# bamCount: k_count, k_count_multi
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("nt", [64, 128, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_count_one_tile_per_workgroup(gpu, layout, nt, heavy):
    _case(gpu, layout, "count", [f"k_count<{nt}> acc=0"] + ([f"k_count<{nt}> acc=1"] if heavy else []), {1: 1}, threads=nt, heavy=heavy)


@pytest.mark.parametrize("residue", [0, 7, 1])
@pytest.mark.parametrize("pre", [2, 3, 4])
@pytest.mark.parametrize("per_wave", [2, 4, 8])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_count_several_tiles_per_wave(gpu, layout, per_wave, pre, residue):
    _case(gpu, layout, "count", [f"k_count_multi<T={per_wave},pre={pre}> acc=0"], {1: per_wave, 2: pre}, threads=64, residue=residue,
          count=True)


# ---------------------------------------------------------------------------------------------------------------
# sums over ranges: k_sum_tiles
# ---------------------------------------------------------------------------------------------------------------
SUMS = [("packed", "sum_half_ss0", "kSumProfile", 0, 1), ("packed", "sum_half_ss1", "kSumProfile", 1, 1)] + \
       [(lay, s, k, ss, 0) for lay in LAYOUTS for s, k, ss in (("sum_word_ss0", "kSumProfile", 0), ("sum_word_ss1", "kSumProfile", 1),
                                                              ("sum_cover", "kSumCover", 0), ("sum_cover_ss", "kSumCoverSS", 1))]


@pytest.mark.parametrize("nw", [1, 2, 4])
@pytest.mark.parametrize("layout,pset,kind,ss,half", SUMS)
def test_sum_tiles(gpu, layout, pset, kind, ss, half, nw):
    """1, 2 and 4 tiles in flight per workgroup; 256-cell tiles, so that the 2,048-bp ranges have eight of them"""
    from bamsignals_amd.device import SumPlan, make_params
    ctx, reads = gpu
    mode, a = deck.gpu_args(pset)
    rg, want = deck.sum_ranges(), deck.expected_sum(pset)
    with _selected({}) as drain:
        plan = SumPlan(ctx, reads[layout], rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(mode, tile_cells=256, threads=64 * nw, **a))
        try:
            first, second, st = plan.run_host().copy(), plan.run_host().copy(), plan.stats()
        finally:
            plan.close()
        names = drain()
    SEEN.update(names)
    assert want.any() and first.dtype == np.int64
    assert np.array_equal(first, want), (names, int(np.sum(first != want)))
    assert np.array_equal(second, want), (names, int(np.sum(second != want)))
    form = f"k_sum_tiles<nw={nw},{kind},ss={ss},half={half},res=%d>"
    assert set(names) == {form % 0, form % 1}, names
    if kind == "kSumProfile":
        assert st["bytes_per_visit_packed"] == (2 if half else 4)
    if half:
        assert st["bytes_per_visit_short"] == 2 and st["visits_short"] > 0


# ---------------------------------------------------------------------------------------------------------------
# the log itself, and the whole list
# ---------------------------------------------------------------------------------------------------------------
def test_log_is_off_by_default_and_empties_itself(gpu):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, reads = gpu
    _, log = _lib_fns()
    buf = ctypes.create_string_buffer(65537)
    rg = deck.ranges()

    def run():
        plan = Plan(ctx, reads["packed"], rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE))
        try:
            plan.run_host()
        finally:
            plan.close()
    assert log(buf, len(buf)) == 0 and buf.value == b""
    run()
    assert log(buf, len(buf)) == 0 and buf.value == b""           # off: nothing was recorded
    with _selected({}) as drain:
        run()
        assert drain() == ["k_coverage<64,pre=2,res=0> acc=0"]
        assert drain() == []                                     # a drain empties it
        run()
    assert log(buf, len(buf)) == 0 and buf.value == b""           # turning it off empties it as well


def test_every_form_was_reached():
    """Runs after the matrix (pytest keeps a module's order): the forms the cases logged are exactly ALL_FORMS."""
    assert len(ALL_FORMS) == len(set(ALL_FORMS))
    # the instantiations behind the names (a name also tells accumulate and the replicas): k_profile 38, k_profile_half 28,
    # k_profile_multi 8, k_profile_multi_half 16, k_profile_small 12, k_coverage 6, k_coverage_bins 12, k_count 3,
    # k_count_multi 9, k_sum_tiles 36
    assert len({n.split("> ")[0] for n in ALL_FORMS}) == 168
    missing, unknown = sorted(set(ALL_FORMS) - SEEN), sorted(SEEN - set(ALL_FORMS))
    assert not missing and not unknown, dict(never_reached=missing, not_listed=unknown)
