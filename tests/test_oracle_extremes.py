"""The checker at megabase shifts and template lengths: the C oracle (chunked queries, int arithmetic as in the
reference, src/bamsignals.cpp:240-291, 339-344) against the all-pairs numpy oracle (int64) on a smaller version of
the inputs of test_parameter_extremes_gpu.py, for every parameter case of that grid, ext = 2^30 included.  The GPU
tests trust oracle_c at exactly these values."""
import numpy as np
import pytest

import extremes_inputs as X


@pytest.fixture(scope="module")
def small():
    from oracle import oracle_c
    cols = X.make_reads(n=20_000, seed=15)
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    return cols, orc


@pytest.fixture(scope="module")
def far():
    from oracle import oracle_c
    cols = X.make_far_reads(n=10_000, seed=16)
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    return cols, orc


def _np_reads(cols):
    return dict(rid=cols["rid"], pos=cols["pos"], end=cols["end"], flag=cols["flag"], mapq=cols["mapq"], tlen=cols["tlen"])


def _same_pileup(cols, orc, rg, **a):
    from oracle import oracle_c, oracle_np
    got, off = oracle_c.pileup_core(orc, rg, **a)
    want, off2 = oracle_np.pileup_core(_np_reads(cols), rg, **a)
    assert np.array_equal(off, off2), a
    assert np.array_equal(got, want), (a, int(np.sum(got != want)))
    return got, off


def _cases():
    for s in X.SHIFTS:
        for b in X.BINSIZES:
            for ss in (False, True):
                yield s, (), None, dict(binsize=b, shift=s, ss=ss)
        for ss in (False, True):
            yield s, (), X.SMALL_TILE_MAX_W, dict(binsize=50, shift=s, ss=ss)
    for s, tf in X.MIDPOINT:
        hs = tuple(h for h in (0, 4_194_304, 5_000_000, 8_388_608, 10_000_000) if h <= tf[1] // 2)
        for b in X.BINSIZES:
            yield s, hs, None, dict(binsize=b, shift=s, ss=True, requiredF=66, pe_mid=True, tlen_filter=tf)
        yield s, hs, X.SMALL_TILE_MAX_W, dict(binsize=50, shift=s, ss=True, requiredF=66, pe_mid=True, tlen_filter=tf)
    for s, tf in X.FILTER_ONLY:
        for b in (-1, 1, 50, 8_193):
            yield s, (), None, dict(binsize=b, shift=s, ss=True, tlen_filter=tf)


def test_oracles_agree_on_the_extremes_grid(small):
    cols, orc = small
    seen = far_rev = 0
    for s, hs, max_w, a in _cases():
        rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, s, hs=hs or (0,), max_w=max_w)
        out, off = _same_pileup(cols, orc, rg, **a)
        seen += X.rev_hits(out, off, rev, rg["strand"], False)[0] > 0
        if a.get("pe_mid"):
            far_rev += X.rev_hits(out, off, rev, rg["strand"], True, min_h=4_194_304)[2] > 0
    assert seen > 100          # (the grid's ranges catch shifted reverse-strand reads, also on this smaller set)
    assert far_rev > 10        # (... and reverse-strand reads moved by midpoints of megabases)


def test_first_mates_of_both_strands_carry_template_lengths():
    """paired.end = "midpoint" with requiredF = 66 keeps first mates only: 99 (forward, tlen > 0) and 83 (reverse,
    tlen < 0); both must carry template lengths of megabases, or no reverse-strand read moves by a midpoint."""
    cols = X.make_reads()
    for f, sgn in ((99, 1), (83, -1), (163, 1), (147, -1)):
        t = cols["tlen"][cols["flag"] == f].astype(np.int64)
        assert len(t) and np.all(np.sign(t) * sgn >= 0) and np.mean(np.abs(t) >= 8_000_000) > 0.25, f
    assert not cols["tlen"][np.isin(cols["flag"], (0, 16))].any()


def test_oracles_agree_on_coverage_with_megabase_spans(small):
    from oracle import oracle_c, oracle_np
    cols, orc = small
    rg, _ = X.place_ranges(X.REFS, X.CLUSTERS, 8_000_000, hs=(0, 4_000_000))
    kw = dict(tspan=True, tlen_filter=X.COVERAGE_TF)
    got, _ = oracle_c.coverage_core(orc, rg, **kw)
    want, _ = oracle_np.coverage_core(_np_reads(cols), rg, **kw)
    assert np.array_equal(got, want)
    assert got.sum() > 0


def test_oracles_agree_at_ext_two_to_the_thirty(far):
    """Shifts of +-(2^30 - 1), +-1e9 and +-2^30 on a 1.2-Gbp reference, and the midpoint with ext = 2^30 exactly."""
    cols, orc = far
    starts = ((0, X.FAR_REF - X.CLUSTER),)
    for s in X.FAR_SHIFTS + (2**30, -2**30):
        rg, rev = X.place_ranges((X.FAR_REF,), starts, s, wrap=False)
        for a in (dict(binsize=1, shift=s), dict(binsize=50, shift=s, ss=True), dict(binsize=-1, shift=s, ss=True)):
            out, off = _same_pileup(cols, orc, rg, **a)
            assert X.rev_hits(out, off, rev, rg["strand"], False)[0] > 0, a
    rg, _ = X.place_ranges((X.FAR_REF,), starts, 2**29, wrap=False)
    out, _ = _same_pileup(cols, orc, rg, binsize=1, shift=2**29, requiredF=66, pe_mid=True, tlen_filter=(0, 2**29), ss=True)
    assert out.sum() > 0
