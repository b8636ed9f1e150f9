"""GPU: the drain of bamProfile's tile image (k_profile, k_profile_half: store_image16) -- the interior vectors of a
tile read from LDS in one batch and stored back to back, the one or two edge vectors in store_vec's form -- cell by cell
against the C oracle.  Ranges of widths 1..9, 255, 256, 257, 2,047 and 2,048 laid out so that every width starts at
each of the four values of out_off & 3 (the image is shifted by that much to line its 16-B vectors up with the
result's), strands merged and split, the looked-up and the resolved form of the launch, 64- and 256-thread workgroups,
the half form and the 4-byte form, and a plan's first and second run (the image is cleared before the item is known).
The register budget of the instantiations the 100,000 x 2-kb launch and its variants take: at most 64 VGPRs, no scratch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = list(range(1, 10)) + [255, 256, 257, 2047, 2048]


@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data(ctx):
    from bamsignals_amd.device import Reads
    from bamsignals_amd.synth import synth_reads
    from oracle import oracle_c
    cols = synth_reads(80_000, [200_000, 50_000], seed=21, with_cigar=False)
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    yield cols, orc, reads
    reads.close()


@pytest.fixture(scope="module")
def ranges(data):
    """280 ranges: every width of WIDTHS twenty times in a seeded order; the flat offset of a range's first cell is the
    sum of the widths in front of it, and every width meets all four of its values mod 4."""
    cols = data[0]
    rng = np.random.default_rng(5)
    width = rng.permutation(np.repeat(np.array(WIDTHS, dtype=np.int32), 20))
    off = np.concatenate([[0], np.cumsum(width[:-1], dtype=np.int64)])
    for w in WIDTHS:
        assert set((off[width == w] & 3).tolist()) == {0, 1, 2, 3}, w
    ref_len = cols["ref_len"]
    rid = rng.integers(0, len(ref_len), len(width)).astype(np.int32)
    loc = (rng.random(len(width)) * (ref_len[rid] - width)).astype(np.int32)
    loc[0], loc[1] = 0, ref_len[rid[1]] - width[1]             # at a reference's first and last base
    strand = rng.choice(np.array([1, -1, 0], dtype=np.int32), len(width))
    return dict(rid=rid, loc=loc, len=width, strand=strand)


def _twice(ctx, reads, rg, threads=0, **a):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_PROFILE, binsize=1, threads=threads, **a))
    try:
        return plan.run_host().copy(), plan.run_host().copy(), plan.stats()
    finally:
        plan.close()


@pytest.mark.parametrize("resolved", [False, True])
@pytest.mark.parametrize("ss", [False, True])
def test_drain_at_every_offset_and_width(ctx, data, ranges, ss, resolved):
    from bamsignals_amd import _lib
    from oracle import oracle_c
    cols, orc, reads = data
    knob = _lib.load().bsig_debug_set_knob
    if resolved:
        assert knob(4, 1) == 0                                   # k_resolve_tiles in front from one tile on
    try:
        # the half form (2 bytes a packed visit) at 64 and 256 threads, the 4-byte form (a filter on mapq) at 64
        for threads, a, bpv in ((0, dict(shift=0), (2,)), (256, dict(shift=-75), (2,)), (0, dict(shift=75, mapqual=10), (4, 8))):
            want, _ = oracle_c.pileup_core(orc, ranges, ss=ss, **a)
            first, second, st = _twice(ctx, reads, ranges, threads=threads, ss=ss, **a)
            assert st["bytes_per_visit_packed"] in bpv, (a, st["bytes_per_visit_packed"])
            assert want.any()
            assert np.array_equal(first, want), (threads, a, int(np.sum(first != want)))
            assert np.array_equal(second, want), (threads, a, int(np.sum(second != want)))
    finally:
        if resolved:
            knob(4, -1)


def test_north_star_kernels_keep_their_register_budget(ctx):
    """k_profile_half<64, ss, passes, 1, resolved> for strands merged with two and one passes in flight and for strands
    split (the kernel-attribute function's cases 7, 8 and 10): at most 64 VGPRs, no scratch."""
    import ctypes
    from bamsignals_amd import _lib
    fn = _lib.load().bsig_debug_pileup_attrs
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    for which in (7, 8, 10):
        regs, scratch = ctypes.c_int(0), ctypes.c_int(-1)
        assert fn(which, ctypes.byref(regs), ctypes.byref(scratch)) == 0, which
        assert scratch.value == 0, (which, scratch.value)
        assert 0 < regs.value <= 64, (which, regs.value)
