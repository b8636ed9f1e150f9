"""GPU: the HIP path against the C oracle, bit for bit, at megabase shifts and template lengths.

The reference takes any int shift and any template-length filter (src/bamsignals.cpp:339-344, 457); a plan takes
ext = |shift| + (midpoint ? tlen_filter[1] : 0) up to 2^30.  The packed class's read bodies work on positions
relative to a chunk (SmallOne::four, CountOne::quad), some with 24-bit multiplies, and every other parity test stops
at shifts of tens of kilobases.  Here the reads sit in clusters on references of 48, 12 and 0.07 Mbp, a third of
them with template lengths of 8-30 Mbp, and the ranges where their shifted 5' ends land (tests/extremes_inputs.py).

Every case runs as a plan run twice (fused, then with its windows resolved in a launch of their own), at 64 and 256
threads, for bamCount with 1-8 tiles per wave, and on the same reads without the packed class (BAMSIGNALS_PACK=0) as
the full-width control; bamCount and the binned forms of binsize 50 and 200 also run in heavy-tile slices of 16 reads.  The oracle must count reads in
the ranges meant for shifted reverse-strand reads: a grid that counts nothing tests nothing.
"""
import numpy as np
import pytest

import extremes_inputs as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _reads(ctx, cols):
    from bamsignals_amd.device import Reads
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                 end=cols["end"])


@pytest.fixture(scope="module")
def data(ctx):
    """The clustered read set, resident twice: with the packed class and without it (every short read in class 0)."""
    from oracle import oracle_c
    mp = pytest.MonkeyPatch()
    cols = X.make_reads()
    packed = _reads(ctx, cols)
    mp.setenv("BAMSIGNALS_PACK", "0")
    try:
        plain = _reads(ctx, cols)
    finally:
        mp.undo()
    assert packed.info()["class_n"][4] > len(cols["pos"]) // 2       # the packed class carries most reads
    assert plain.info()["class_n"][4] == 0
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    yield dict(cols=cols, packed=packed, plain=plain, orc=orc)
    packed.close()
    plain.close()


def _mode(kind, a):
    from bamsignals_amd import _lib
    if kind == "coverage":
        return _lib.MODE_COVERAGE_EX if "binsize" in a else _lib.MODE_COVERAGE
    return _lib.MODE_COUNT if a.get("binsize", 1) <= 0 else _lib.MODE_PROFILE


def _plan_runs(ctx, reads, rg, kind, a, threads=0):
    """Both forms of one plan: its first run (fused) and its second (windows resolved by k_resolve_tiles)."""
    from bamsignals_amd.device import Plan, make_params
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_mode(kind, a), threads=threads, **a))
    try:
        return [plan.run_host(), plan.run_host()]
    finally:
        plan.close()


def _forms(ctx, data, rg, kind, a, heavy=False):
    """(form name, result) of every way the HIP path can run this case."""
    from bamsignals_amd import _lib
    out = []
    for th in (64, 256):
        for k, r in enumerate(_plan_runs(ctx, data["packed"], rg, kind, a, threads=th)):
            out.append(("threads=%d run=%d" % (th, k + 1), r))
    if kind == "pileup" and a["binsize"] <= 0:
        knob = _lib.load().bsig_debug_set_knob
        try:
            for tiles in (1, 2, 4, 8):
                assert knob(1, tiles) == 0
                for k, r in enumerate(_plan_runs(ctx, data["packed"], rg, kind, a)):
                    out.append(("tiles/wave=%d run=%d" % (tiles, k + 1), r))
        finally:
            knob(1, 0)
    if heavy:
        mp = pytest.MonkeyPatch()
        mp.setenv("BAMSIGNALS_HEAVY_READS", "64")
        try:
            for k, r in enumerate(_plan_runs(ctx, data["packed"], rg, kind, a)):
                out.append(("heavy=64 run=%d" % (k + 1), r))
        finally:
            mp.undo()
    for k, r in enumerate(_plan_runs(ctx, data["plain"], rg, kind, a)):
        out.append(("PACK=0 run=%d" % (k + 1), r))
    return out


def _summary(bad):
    """Failing cases, one line each: the parameters and the forms that differ from the oracle (cells that differ)."""
    by = {}
    for a, form, n in bad:
        by.setdefault(repr(sorted(a.items())), []).append("%s: %d" % (form, n))
    return "\n".join("%s -> %s" % (k, "; ".join(v)) for k, v in by.items())


def _check(ctx, data, rg, rev, kind, a, want, off, bad, heavy=False, far_h=None):
    """Compare every form with `want`; a mismatch goes into `bad` as (parameters, form, cells that differ).
    `rev` (None: no such check): the oracle must count reads in the ranges meant for reverse-strand reads; with
    `far_h`, reverse-strand reads themselves in the ranges placed for midpoints h >= far_h (strand-split cases)."""
    if rev is not None:
        tot, anti, _ = X.rev_hits(want, off, rev, rg["strand"], a.get("ss", False))
        assert tot > 0, ("no reverse-strand read reaches its ranges", a)
        if a.get("ss"):
            assert anti > 0, ("antisense row empty", a)
        if far_h is not None:
            assert X.rev_hits(want, off, rev, rg["strand"], True, min_h=far_h)[2] > 0, \
                ("no reverse-strand read moved by a midpoint >= %d" % far_h, a)
    for form, got in _forms(ctx, data, rg, kind, a, heavy=heavy):
        if got.shape != want.shape or not np.array_equal(got, want):
            n = int(np.sum(got != want)) if got.shape == want.shape else -1
            bad.append((dict(a), form, n))


@pytest.mark.parametrize("shift", X.SHIFTS)
def test_profile_and_count_at_shift(ctx, data, shift):
    """bamProfile at binsize 1 (ProfileOne's mod-2^32 body), 2 and 50 (k_profile's read-by-read form: ranges of up to
    40,000 bases make tiles of more than 256 values), 200 and 8,192 (k_profile_small, SmallOne, on both sides of its
    narrow form's 32,768-base edge; 8,192: the widest bins it takes), 8,193 and 50,000 (bins as count items) and
    bamCount, with and without strand split; and binsize 50 on ranges of at most 5,000 bases (k_profile_small: the
    "bins of 50-500 bp" form)."""
    from oracle import oracle_c
    rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, shift)
    small, small_rev = X.place_ranges(X.REFS, X.CLUSTERS, shift, max_w=X.SMALL_TILE_MAX_W)
    bad = []
    for b in X.BINSIZES:
        for ss in (False, True):
            a = dict(binsize=b, shift=shift, ss=ss)
            want, off = oracle_c.pileup_core(data["orc"], rg, **a)
            _check(ctx, data, rg, rev, "pileup", a, want, off, bad, heavy=ss and b in (-1, 50, 200))
    for ss in (False, True):
        a = dict(binsize=50, shift=shift, ss=ss)
        want, off = oracle_c.pileup_core(data["orc"], small, **a)
        _check(ctx, data, small, small_rev, "pileup", a, want, off, bad, heavy=ss)
    assert not bad, _summary(bad)


FAR_H = 4_194_304      # midpoints from here on put a reverse-strand read's 24-bit operand out of range at shift 0


def _hs(tf1):
    return tuple(h for h in (0, 4_194_304, 5_000_000, 8_388_608, 10_000_000) if h <= tf1 // 2)


@pytest.mark.parametrize("shift,tf", X.MIDPOINT, ids=lambda v: str(v))
def test_midpoint_at_megabase_template_lengths(ctx, data, shift, tf):
    """paired.end = "midpoint" (requiredF = 66) with filters up to (0, 1e9): the 5' end moves by |tlen| >> 1 of
    up to 10 Mbp; with (0, 1e9) ext is about 2^30, with (0, 2^30 - 4,177,000) and shift 4,177,000 exactly 2^30, and
    every window is clipped to its reference.
    Reverse-strand reads moved by midpoints of 4.19 Mbp and more must reach their ranges."""
    from oracle import oracle_c
    hs = _hs(tf[1])
    assert max(hs) >= FAR_H
    rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, shift, hs=hs)
    small, small_rev = X.place_ranges(X.REFS, X.CLUSTERS, shift, hs=hs, max_w=X.SMALL_TILE_MAX_W)
    bad = []
    for b in X.BINSIZES:
        a = dict(binsize=b, shift=shift, ss=True, requiredF=66, pe_mid=True, tlen_filter=tf)
        want, off = oracle_c.pileup_core(data["orc"], rg, **a)
        _check(ctx, data, rg, rev, "pileup", a, want, off, bad, heavy=b in (-1, 50, 200), far_h=FAR_H)
    a = dict(binsize=50, shift=shift, ss=True, requiredF=66, pe_mid=True, tlen_filter=tf)
    want, off = oracle_c.pileup_core(data["orc"], small, **a)
    _check(ctx, data, small, small_rev, "pileup", a, want, off, bad, heavy=True, far_h=FAR_H)
    assert not bad, _summary(bad)


@pytest.mark.parametrize("shift,tf", X.FILTER_ONLY, ids=lambda v: str(v))
def test_template_length_filter_only(ctx, data, shift, tf):
    """A filter that keeps |tlen| in {8,000,000, 8,000,001} only, without the midpoint rule."""
    from oracle import oracle_c
    rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, shift)
    bad = []
    for b in (-1, 1, 50, 8_193):
        a = dict(binsize=b, shift=shift, ss=True, tlen_filter=tf)
        want, off = oracle_c.pileup_core(data["orc"], rg, **a)
        _check(ctx, data, rg, rev, "pileup", a, want, off, bad)
    assert not bad, _summary(bad)


def _coverage_expected(cols, rg, b, ss, **kw):
    """The oracle's per-base coverage, binned and split by strand here (as test_coverage_binned_gpu.py does)."""
    from oracle import oracle_c
    ref_off = np.asarray(cols["ref_off"], np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))

    def per_base(mask):
        counts = np.bincount(rid[mask], minlength=len(ref_off) - 1)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        o = oracle_c.OracleReads(off, cols["pos"][mask], cols["end"][mask], cols["flag"][mask], cols["mapq"][mask],
                                 cols["tlen"][mask])
        out, offs = oracle_c.coverage_core(o, rg, **kw)
        return [out[offs[i]:offs[i + 1]].astype(np.int64) for i in range(len(rg["rid"]))]

    def binned(v):
        return np.add.reduceat(v, np.arange(0, len(v), b)) if len(v) else np.zeros(0, np.int64)

    fwd = (np.asarray(cols["flag"]) & 16) == 0
    if not ss:
        return np.concatenate([binned(v) for v in per_base(np.ones(len(fwd), bool))])
    parts = []
    for i, (f, r) in enumerate(zip(per_base(fwd), per_base(~fwd))):
        sense, anti = (r, f) if rg["strand"][i] < 0 else (f, r)
        parts.append(np.stack([binned(sense), binned(anti)]).T.reshape(-1))
    return np.concatenate(parts)


def test_coverage_with_megabase_template_spans(ctx, data):
    """bamCoverage(paired.end = "extend") with tlen_filter (0, 2e7): reads cover up to 20 Mbp, ext = 2e7; per base
    (k_coverage) and in 50-bp bins split by strand (k_coverage_bins)."""
    from oracle import oracle_c
    cols = data["cols"]
    rg, _ = X.place_ranges(X.REFS, X.CLUSTERS, 8_000_000, hs=(0, 4_000_000))
    kw = dict(tspan=True, tlen_filter=X.COVERAGE_TF)
    bad = []
    want, off = oracle_c.coverage_core(data["orc"], rg, **kw)
    # ranges megabases from every cluster are covered by template spans alone
    starts = np.asarray([c for cl in X.CLUSTERS for c in cl], np.int64)
    lone = [i for i in range(len(rg["rid"])) if np.abs(starts - int(rg["loc"][i])).min() > 1_000_000]
    assert sum(int(want[off[i]:off[i + 1]].sum()) > 0 for i in lone) > 5
    _check(ctx, data, rg, None, "coverage", kw, want, off, bad)
    want50 = _coverage_expected(cols, rg, 50, True, **kw).astype(np.int32)
    assert int(want50[1::2].sum()) > 0
    _check(ctx, data, rg, None, "coverage", dict(kw, binsize=50, ss=True), want50, None, bad)
    assert not bad, _summary(bad)


def test_far_shifts_on_a_gigabase_reference(ctx):
    """One 1.2-Gbp reference with reads near both ends: shifts of +-(2^30 - 1) and +-1e9 move them from one end to
    the other (profile, 50-bp bins, count); ext = 2^30 exactly is taken, 2^30 + 1 is refused."""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    from oracle import oracle_c
    cols = X.make_far_reads()
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    reads = _reads(ctx, cols)
    mp = pytest.MonkeyPatch()
    mp.setenv("BAMSIGNALS_PACK", "0")
    try:
        plain = _reads(ctx, cols)
    finally:
        mp.undo()
    data = dict(packed=reads, plain=plain)
    bad = []
    try:
        for shift in X.FAR_SHIFTS + (2**30, -2**30):
            rg, rev = X.place_ranges((X.FAR_REF,), ((0, X.FAR_REF - X.CLUSTER),), shift, wrap=False)
            for a in (dict(binsize=1, shift=shift), dict(binsize=50, shift=shift, ss=True), dict(binsize=-1, shift=shift, ss=True)):
                want, off = oracle_c.pileup_core(orc, rg, **a)
                _check(ctx, data, rg, rev, "pileup", a, want, off, bad)
        # midpoint: ext = |shift| + tf1 = 2^30 exactly
        rg, _ = X.place_ranges((X.FAR_REF,), ((0, X.FAR_REF - X.CLUSTER),), 2**29, wrap=False)
        a = dict(binsize=1, shift=2**29, requiredF=66, pe_mid=True, tlen_filter=(0, 2**29), ss=True)
        want, _ = oracle_c.pileup_core(orc, rg, **a)
        assert want.sum() > 0
        _check(ctx, data, rg, None, "pileup", a, want, None, bad)
        assert not bad, _summary(bad)
        # one base more is refused, by shift and by the filter alike
        for a in (dict(binsize=1, shift=2**30 + 1), dict(binsize=-1, shift=-(2**30 + 1)),
                  dict(binsize=1, shift=2**29 + 1, requiredF=66, pe_mid=True, tlen_filter=(0, 2**29))):
            with pytest.raises(_lib.BsigError, match="shift / tlen filter too large") as e:
                Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_mode("pileup", a), **a))
            assert e.value.code_name == "BSIG_ERR_ARG"
    finally:
        reads.close()
        plain.close()


def test_file_level_calls_at_a_megabase_shift(ctx, data, tmp_path):
    """bamCount and bamProfile(binsize = 50, ss = True) at shift 5e6 on a BAM written by this package's writer (the
    profile on ranges of at most 5,000 bases: k_profile_small)."""
    from bamsignals_amd import GRanges, bamCount, bamProfile, write_columns_as_bam
    from oracle import oracle_c
    cols = data["cols"]
    names = ["chrA", "chrB", "chrC"]
    bam = str(tmp_path / "extremes.bam")
    write_columns_as_bam(bam, names, cols)
    rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, 5_000_000)
    gr = GRanges([names[r] for r in rg["rid"]], rg["loc"] + 1, width=rg["len"],
                 strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in rg["strand"]])
    want_c, off = oracle_c.pileup_core(data["orc"], rg, binsize=-1, shift=5_000_000)
    assert X.rev_hits(want_c, off, rev, rg["strand"], False)[0] > 0
    assert np.array_equal(bamCount(bam, gr, shift=5_000_000, verbose=False), want_c)
    rg, rev = X.place_ranges(X.REFS, X.CLUSTERS, 5_000_000, max_w=X.SMALL_TILE_MAX_W)
    gr = GRanges([names[r] for r in rg["rid"]], rg["loc"] + 1, width=rg["len"],
                 strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in rg["strand"]])
    want_p, off = oracle_c.pileup_core(data["orc"], rg, binsize=50, ss=True, shift=5_000_000)
    assert X.rev_hits(want_p, off, rev, rg["strand"], True)[1] > 0
    p = bamProfile(bam, gr, binsize=50, ss=True, shift=5_000_000, verbose=False)
    assert np.array_equal(np.concatenate([m.T.reshape(-1) for m in p]), want_p)
