"""GPU: bamProfile's half form -- the packed class read from its 16-bit 5'-end column (k_profile_half,
k_profile_multi_half) -- bit for bit against the C oracle and against the 4-byte form (the same reads made with
BAMSIGNALS_PACKED_HALF=0), and the plans that must or must not take it (plan.stats()["bytes_per_visit_packed"]: 2 for
the half form).  Forward, reverse and '*' ranges, strands merged and split, shifts up to the window bound and one past
it, reads and ranges at reference ends, 500-bp / 1-kb / 2-kb tiles, a pileup cut into heavy-tile slices, a file with
more than 512 (flag, mapq) pairs, and reads that come through bsig_reads_load and bsig_reads_clone."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _columns(seed, n, many_pairs=False, pile=0):
    """Single-end synthetic reads on three references; reads at every reference's first and last base; `pile` extra
    reads on 60 bases of reference 0; with `many_pairs` about 1,900 (flag, mapq) pairs."""
    from bamsignals_amd.synth import synth_reads
    c = synth_reads(n, [400_000, 150_000, 30_000], seed=seed, with_cigar=False)
    rid, pos, end, flag, mapq, tlen = c["rid"], c["pos"], c["end"], c["flag"], c["mapq"], c["tlen"]
    rng = np.random.default_rng(seed)
    extra = []
    for r, L in enumerate(c["ref_len"]):
        for p in (0, 0, 1, int(L) - 1, int(L) - 1, int(L) - 2):
            extra.append((r, p, p + int(rng.integers(0, 256)), int(rng.choice([0, 16]))))
    for _ in range(pile):
        p = 200_000 + int(rng.integers(0, 60))
        extra.append((0, p, p + 99, int(rng.choice([0, 16]))))
    e = np.array(extra, dtype=np.int64)
    rid = np.concatenate([rid, e[:, 0]]).astype(np.int32)
    pos = np.concatenate([pos, e[:, 1]]).astype(np.int32)
    end = np.concatenate([end, e[:, 2]]).astype(np.int32)
    flag = np.concatenate([flag, e[:, 3]]).astype(np.uint16)
    mapq = np.concatenate([mapq, rng.integers(0, 61, len(e))]).astype(np.uint8)
    tlen = np.concatenate([tlen, np.zeros(len(e))]).astype(np.int32)
    if many_pairs:
        # secondary / QC-fail / supplementary / paired bits on a third of the reads: 32 flags x 61 mapq values
        bits = np.array([0x100, 0x200, 0x800, 0x1, 0x40], dtype=np.uint16)
        pick = rng.random((len(flag), len(bits))) < 0.33
        flag = (flag | (pick * bits).sum(axis=1).astype(np.uint16)).astype(np.uint16)
    o = np.lexsort((pos, rid))
    rid, pos, end, flag, mapq, tlen = rid[o], pos[o], end[o], flag[o], mapq[o], tlen[o]
    ref_off = np.searchsorted(rid, np.arange(len(c["ref_len"]) + 1)).astype(np.int64)
    return dict(ref_len=c["ref_len"], ref_off=ref_off, rid=rid, pos=pos, end=end, flag=flag, mapq=mapq, tlen=tlen)


def _make(ctx, cols, half=True):
    from bamsignals_amd.device import Reads
    old = os.environ.get("BAMSIGNALS_PACKED_HALF")
    if half:
        os.environ.pop("BAMSIGNALS_PACKED_HALF", None)
    else:
        os.environ["BAMSIGNALS_PACKED_HALF"] = "0"
    try:
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    finally:
        if old is None:
            os.environ.pop("BAMSIGNALS_PACKED_HALF", None)
        else:
            os.environ["BAMSIGNALS_PACKED_HALF"] = old


@pytest.fixture(scope="module")
def data(ctx):
    from oracle import oracle_c
    cols = _columns(11, 300_000, pile=40_000)
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    half, full = _make(ctx, cols, True), _make(ctx, cols, False)
    yield cols, orc, half, full
    half.close(); full.close()


def _ranges(cols, width, n, seed):
    rng = np.random.default_rng(seed)
    ref_len = cols["ref_len"]
    rid = rng.integers(0, len(ref_len), n).astype(np.int32)
    loc = (rng.random(n) * (ref_len[rid] - width // 2)).astype(np.int32)
    loc[:3] = 0                                         # at reference starts ...
    loc[3:6] = ref_len[rid[3:6]] - width                # ... ends ...
    loc[6:9] = ref_len[rid[6:9]] - width // 3           # ... and clipped by them
    strand = rng.choice(np.array([1, -1, 0], dtype=np.int32), n)
    return dict(rid=rid, loc=loc, len=np.full(n, width, dtype=np.int32), strand=strand)


def _run(ctx, reads, rg, threads=0, **a):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    bs = a.pop("binsize", 1)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_PROFILE, binsize=bs, threads=threads, **a))
    try:
        return plan.run_host(), plan.stats()
    finally:
        plan.close()


def _check(ctx, orc, half, full, rg, bpv, threads=0, **a):
    from oracle import oracle_c
    want, _ = oracle_c.pileup_core(orc, rg, **a)
    got, st = _run(ctx, half, rg, threads=threads, **dict(a))
    assert st["bytes_per_visit_packed"] in (bpv if isinstance(bpv, tuple) else (bpv,)), (a, st["bytes_per_visit_packed"])
    assert np.array_equal(got, want), (a, int(np.sum(got != want)))
    if full is not None:
        got4, st4 = _run(ctx, full, rg, threads=threads, **dict(a))
        assert st4["bytes_per_visit_packed"] in (4, 8), a
        assert np.array_equal(got4, got), a
    return st


@pytest.mark.parametrize("width", [500, 1000, 2000])
def test_half_form_matches_oracle_and_the_4_byte_form(ctx, data, width):
    cols, orc, half, full = data
    rg = _ranges(cols, width, 3000, seed=width)
    for shift in (0, 75, -75, 5000, -5000):
        for ss in (False, True):
            _check(ctx, orc, half, full, rg, 2, shift=shift, ss=ss)
    # past the window bound (tile + 2 |shift| + maxspan + buckets > 2^15 - 256): the 4-byte form, still exact
    for shift in (16_200, -16_200):
        _check(ctx, orc, half, full, rg, 4, shift=shift, ss=True)


def test_half_form_in_large_launches_and_wider_workgroups(ctx, data):
    """k_resolve_tiles in front from one tile on (k_profile_multi_half for 500-bp tiles, the resolved k_profile_half
    otherwise), both passes-in-flight builds, 256-thread workgroups."""
    from bamsignals_amd import _lib
    cols, orc, half, full = data
    knob = _lib.load().bsig_debug_set_knob
    try:
        assert knob(4, 1) == 0
        for pre in (1, 2):
            assert knob(6, pre) == 0
            for width in (500, 2000):
                rg = _ranges(cols, width, 2000, seed=width + 7)
                for shift, ss in ((0, False), (-75, True), (5000, True)):
                    _check(ctx, orc, half, full, rg, 2, shift=shift, ss=ss)
    finally:
        knob(4, -1)
        knob(6, 2)
    rg = _ranges(cols, 2000, 1000, seed=99)
    _check(ctx, orc, half, full, rg, 2, threads=256, shift=75, ss=True)


def test_half_form_heavy_tiles(ctx, data):
    """40,000 reads on 60 bases: the tiles over them are cut into slices that add up with atomics."""
    cols, orc, half, full = data
    rg = _ranges(cols, 2000, 50, seed=5)
    rg["rid"][:10] = 0
    rg["loc"][:10] = 200_000 - np.arange(10, dtype=np.int32) * 150
    for ss in (False, True):
        st = _check(ctx, orc, half, full, rg, 2, shift=-30, ss=ss)
        assert st["heavy_tiles"] > 0


def test_plans_that_keep_the_4_byte_form(ctx, data):
    cols, orc, half, _ = data
    rg = _ranges(cols, 1000, 1000, seed=3)
    for a in (dict(mapqual=10), dict(requiredF=1), dict(filteredF=16), dict(tlen_filter=(0, 1000)),
              dict(tlen_filter=(0, 1000), pe_mid=True), dict(binsize=2), dict(shift=20_000)):
        _check(ctx, orc, half, None, rg, (4, 8), **a)           # (8: the word and its tlen)


def test_half_form_with_class_0(ctx):
    """More than 512 (flag, mapq) pairs: the rarer ones stay in class 0, the rest takes the half form."""
    from oracle import oracle_c
    cols = _columns(12, 200_000, many_pairs=True)
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    half, full = _make(ctx, cols, True), _make(ctx, cols, False)
    try:
        inf = half.info()
        assert inf["n_codes"] == 512 and inf["class_n"][0] > 0 and inf["class_n"][4] > 0
        rg = _ranges(cols, 2000, 2000, seed=4)
        for shift, ss in ((0, False), (75, True), (-5000, True)):
            _check(ctx, orc, half, full, rg, 2, shift=shift, ss=ss)
        # (a rejecting filter keeps the 4-byte form here too)
        _check(ctx, orc, half, full, rg, 4, requiredF=0x100)
    finally:
        half.close(); full.close()


def test_half_form_after_load_and_clone(ctx, data, tmp_path, monkeypatch):
    """bsig_reads_load and bsig_reads_clone derive the column again (it is never saved); with
    BAMSIGNALS_PACKED_HALF=0 they leave it out."""
    from bamsignals_amd.device import Reads
    cols, orc, half, _ = data
    path = str(tmp_path / "r.bsig")
    half.save(path, "s")
    rg = _ranges(cols, 2000, 1500, seed=8)
    hbm = {}
    for how in ("load", "clone"):
        r = Reads.load(ctx, path, "s") if how == "load" else half.clone(ctx)
        try:
            _check(ctx, orc, r, None, rg, 2, shift=75, ss=True)
            hbm[how] = r.info()["hbm_bytes"]
        finally:
            r.close()
    monkeypatch.setenv("BAMSIGNALS_PACKED_HALF", "0")
    n_packed = half.info()["class_n"][4]
    for how in ("load", "clone"):
        r = Reads.load(ctx, path, "s") if how == "load" else half.clone(ctx)
        try:
            _check(ctx, orc, r, None, rg, 4, shift=75, ss=True)
            assert hbm[how] - r.info()["hbm_bytes"] >= 2 * n_packed, how
        finally:
            r.close()


def test_half_kernels_keep_their_register_budget(ctx):
    """No scratch and at most 64 VGPRs for the half form's kernels (k_profile_half with two and one passes in flight,
    k_profile_multi_half, strands split)."""
    import ctypes
    from bamsignals_amd import _lib
    fn = _lib.load().bsig_debug_pileup_attrs
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    base = ctypes.c_int(0), ctypes.c_int(-1)
    assert fn(0, ctypes.byref(base[0]), ctypes.byref(base[1])) == 0
    for which in (7, 8, 9, 10):
        regs, scratch = ctypes.c_int(0), ctypes.c_int(-1)
        assert fn(which, ctypes.byref(regs), ctypes.byref(scratch)) == 0, which
        assert scratch.value == 0, (which, scratch.value)
        assert 0 < regs.value <= 64, (which, regs.value)
    regs = ctypes.c_int(0)
    assert fn(7, ctypes.byref(regs), None) == 0 and regs.value <= base[0].value
