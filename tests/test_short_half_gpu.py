"""GPU: span classes 0 and 1 read from their 16-bit 5'-end columns (BsigKParams::short_half; for_each_read<..., HALF>
with ProfileOne::half1 / oct) -- every case bit for bit against the C oracle and against the same reads made with
BAMSIGNALS_SHORT_HALF=0 (the pos + fm path), and plan.stats()["bytes_per_visit_short"] says which path a plan takes:
2 for the columns, 8 for pos + fm.

The reads are those of test_packed_half_gpu.py (300,000 single-end reads on references of 400,000 / 150,000 / 30,000
bases, about 2.5 % of them class 1) and, added to them: reads of span 1 and 4,096 on both strands at every reference's
first and last base; on a stretch of reference 0 cleared of other class-1 reads, islands of exactly 63, 64, 65 and 600
class-1 reads inside one 2-kb tile (one read per lane up to 64, the eight-read loop beyond) and eight islands of 73
whose windows start at every residue modulo 8; a pile that makes heavy tiles.  `many_pairs` gives class 0."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ISLAND_REF = 0
ISLAND_LO, ISLAND_STEP = 20_000, 9_000                  # island k lies in the tile [ISLAND_LO + k * ISLAND_STEP, + 2,000)
ISLAND_SIZES = (63, 64, 65, 600) + (73,) * 8            # (73 = 1 mod 8: every island's window starts one residue further)
CLEARED = (8_000, ISLAND_LO + len(ISLAND_SIZES) * ISLAND_STEP + 4_000)


@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _columns(seed, n, many_pairs=False, pile=0):
    from bamsignals_amd.synth import synth_reads
    c = synth_reads(n, [400_000, 150_000, 30_000], seed=seed, with_cigar=False)
    rid, pos, end, flag, mapq, tlen = c["rid"], c["pos"], c["end"], c["flag"], c["mapq"], c["tlen"]
    rng = np.random.default_rng(seed)
    # no read longer than 256 bases near the islands but theirs
    keep = ~((rid == ISLAND_REF) & (pos >= CLEARED[0]) & (pos < CLEARED[1]) & (end - pos + 1 > 256))
    rid, pos, end, flag, mapq, tlen = rid[keep], pos[keep], end[keep], flag[keep], mapq[keep], tlen[keep]
    extra = []                                           # (rid, pos, end, flag)
    for r, L in enumerate(c["ref_len"]):
        for p in (0, int(L) - 1):
            for span in (1, 4096):
                for f in (0, 16):
                    extra.append((r, p, p + span - 1, f))
        for p in (0, 1, int(L) - 1, int(L) - 2):
            extra.append((r, p, p + int(rng.integers(0, 256)), int(rng.choice([0, 16]))))
    for k, m in enumerate(ISLAND_SIZES):
        t0 = ISLAND_LO + k * ISLAND_STEP
        for p in np.sort(rng.integers(t0 + 100, t0 + 1900, m)):
            extra.append((ISLAND_REF, int(p), int(p) + int(rng.integers(257, 1500)) - 1, int(rng.choice([0, 16]))))
    for _ in range(pile):
        p = 300_000 + int(rng.integers(0, 60))
        extra.append((0, p, p + int(rng.choice([99, 299])), int(rng.choice([0, 16]))))
    e = np.array(extra, dtype=np.int64)
    rid = np.concatenate([rid, e[:, 0]]).astype(np.int32)
    pos = np.concatenate([pos, e[:, 1]]).astype(np.int32)
    end = np.concatenate([end, e[:, 2]]).astype(np.int32)
    flag = np.concatenate([flag, e[:, 3]]).astype(np.uint16)
    mapq = np.concatenate([mapq, rng.integers(0, 61, len(e))]).astype(np.uint8)
    tlen = np.concatenate([tlen, np.zeros(len(e))]).astype(np.int32)
    if many_pairs:
        bits = np.array([0x100, 0x200, 0x800, 0x1, 0x40], dtype=np.uint16)
        pick = rng.random((len(flag), len(bits))) < 0.33
        flag = (flag | (pick * bits).sum(axis=1).astype(np.uint16)).astype(np.uint16)
    o = np.lexsort((pos, rid))
    rid, pos, end, flag, mapq, tlen = rid[o], pos[o], end[o], flag[o], mapq[o], tlen[o]
    ref_off = np.searchsorted(rid, np.arange(len(c["ref_len"]) + 1)).astype(np.int64)
    return dict(ref_len=c["ref_len"], ref_off=ref_off, rid=rid, pos=pos, end=end, flag=flag, mapq=mapq, tlen=tlen)


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def _make(ctx, cols, short=True):
    from bamsignals_amd.device import Reads
    with _env("BAMSIGNALS_SHORT_HALF", None if short else "0"):
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])


class _Data:
    def __init__(self, ctx, seed, n, **kw):
        from oracle import oracle_c
        self.cols = _columns(seed, n, **kw)
        c = self.cols
        self.orc = oracle_c.OracleReads(c["ref_off"], c["pos"], c["end"], c["flag"], c["mapq"], c["tlen"])
        self.on, self.off = _make(ctx, c, True), _make(ctx, c, False)
        self.want = {}                                   # the oracle's answers, one per (ranges, arguments)

    def oracle(self, key, rg, **a):
        from oracle import oracle_c
        k = (key, tuple(sorted(a.items())))
        if k not in self.want:
            self.want[k] = oracle_c.pileup_core(self.orc, rg, **a)[0]
        return self.want[k]

    def close(self):
        self.on.close(); self.off.close()


@pytest.fixture(scope="module")
def data(ctx):
    d = _Data(ctx, 11, 300_000, pile=40_000)
    yield d
    d.close()


@pytest.fixture(scope="module")
def data0(ctx):
    d = _Data(ctx, 12, 200_000, many_pairs=True)
    yield d
    d.close()


def _ranges(cols, width, n, seed):
    rng = np.random.default_rng(seed)
    ref_len = cols["ref_len"]
    rid = rng.integers(0, len(ref_len), n).astype(np.int32)
    loc = (rng.random(n) * (ref_len[rid] - width // 2)).astype(np.int32)
    loc[:3] = 0                                         # at reference starts ...
    loc[3:6] = ref_len[rid[3:6]] - width                # ... ends ...
    loc[6:9] = ref_len[rid[6:9]] - width // 3           # ... and clipped by them
    k = np.arange(len(ISLAND_SIZES))                    # ... and the islands' tiles
    rid[9:9 + len(k)] = ISLAND_REF
    loc[9:9 + len(k)] = ISLAND_LO + k * ISLAND_STEP
    strand = rng.choice(np.array([1, -1, 0], dtype=np.int32), n)
    return dict(rid=rid, loc=loc, len=np.full(n, width, dtype=np.int32), strand=strand)


def _run(ctx, reads, rg, threads=0, **a):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_PROFILE, threads=threads, **a))
    try:
        return plan.run_host(), plan.stats()
    finally:
        plan.close()


def _check(ctx, d, key, rg, bpv_short, bpv_packed=2, threads=0, **a):
    want = d.oracle(key, rg, **a)
    got, st = _run(ctx, d.on, rg, threads=threads, **a)
    assert st["bytes_per_visit_short"] == bpv_short, (a, st["bytes_per_visit_short"])
    assert st["bytes_per_visit_packed"] == bpv_packed, (a, st["bytes_per_visit_packed"])
    assert np.array_equal(got, want), (a, int(np.sum(got != want)))
    got8, st8 = _run(ctx, d.off, rg, threads=threads, **a)
    assert st8["bytes_per_visit_short"] == 8, a
    assert np.array_equal(got8, got), a
    return st


def test_the_islands_hold_what_they_claim(ctx, data):
    """One 2-kb range per island: the class-0/1 visits of its plan are its window, the island's own reads and no other
    (class 0 is empty here: every short read's pair has a code)."""
    inf = data.on.info()
    assert inf["class_n"][0] == 0 and inf["class_n"][1] > 5000
    for k, m in enumerate(ISLAND_SIZES):
        rg = dict(rid=np.array([ISLAND_REF], dtype=np.int32), loc=np.array([ISLAND_LO + k * ISLAND_STEP], dtype=np.int32),
                  len=np.array([2000], dtype=np.int32), strand=np.array([1], dtype=np.int32))
        st = _check(ctx, data, ("island", k), rg, 2, shift=0, ss=False)       # (strands merged: the range is ONE tile)
        assert st["n_items"] == 1 and st["visits_short"] == m, (k, m, st["visits_short"])
        _check(ctx, data, ("island", k), rg, 2, shift=0, ss=True)


@pytest.mark.parametrize("width", [500, 1000, 2000])
def test_short_columns_match_oracle_and_the_pos_fm_path(ctx, data, width):
    rg = _ranges(data.cols, width, 3000, seed=width)
    for shift in (0, 75, -75, 5000, -5000):
        for ss in (False, True):
            _check(ctx, data, width, rg, 2, shift=shift, ss=ss)


def test_short_columns_with_class_0(ctx, data0):
    inf = data0.on.info()
    assert inf["n_codes"] == 512 and inf["class_n"][0] > 0 and inf["class_n"][1] > 0 and inf["class_n"][4] > 0
    rg = _ranges(data0.cols, 2000, 2000, seed=4)
    for shift, ss in ((0, False), (75, True), (-5000, True)):
        _check(ctx, data0, "c0", rg, 2, shift=shift, ss=ss)
    rg = _ranges(data0.cols, 500, 2000, seed=5)
    _check(ctx, data0, "c0w", rg, 2, shift=-75, ss=True)


def test_short_columns_in_large_launches_and_wider_workgroups(ctx, data):
    """Knob 4 = 1: k_resolve_tiles in front from one tile on (k_profile_multi_half for 500-bp tiles, the resolved
    k_profile_half otherwise), with one and two passes in flight (knob 6); 256-thread workgroups (there a window of up
    to 256 reads is one read per lane: the 600-read island alone takes the eight-read loop)."""
    from bamsignals_amd import _lib
    knob = _lib.load().bsig_debug_set_knob
    try:
        assert knob(4, 1) == 0
        for pre in (1, 2):
            assert knob(6, pre) == 0
            for width in (500, 2000):
                rg = _ranges(data.cols, width, 2000, seed=width + 7)
                for shift, ss in ((0, False), (-75, True), (5000, True)):
                    _check(ctx, data, ("k", width), rg, 2, shift=shift, ss=ss)
    finally:
        knob(4, -1)
        knob(6, 2)
    rg = _ranges(data.cols, 2000, 1000, seed=99)
    _check(ctx, data, "t256", rg, 2, threads=256, shift=75, ss=True)


def test_short_columns_heavy_tiles(ctx, data):
    """40,000 reads on 60 bases, half of them class 1: tiles cut into slices, whose fixed read ranges of class 1 take
    the columns with their tile's base."""
    rg = _ranges(data.cols, 2000, 50, seed=5)
    rg["rid"][:9] = 0
    rg["loc"][:9] = 300_000 - np.arange(9, dtype=np.int32) * 150
    for ss in (False, True):
        st = _check(ctx, data, "heavy", rg, 2, shift=-30, ss=ss)
        assert st["heavy_tiles"] > 0


def test_plans_that_keep_pos_and_fm(ctx, data):
    """A filter that could reject a read keeps classes 0 and 1 on pos + fm (the packed class goes by the file's codes:
    filteredF=0x200 rejects none of them here), and so does a shift just past class 1's window bound but inside the
    packed class's."""
    rg = _ranges(data.cols, 1000, 1000, seed=3)
    for a, packed in ((dict(mapqual=10), 4), (dict(requiredF=1), 4), (dict(filteredF=16), 4), (dict(filteredF=0x200), 2)):
        _check(ctx, data, "fb", rg, 8, bpv_packed=packed, **a)
    inf = data.on.info()
    m1, k1 = inf["class_maxspan"][1], inf["class_bucket_shift"][1]
    m4, k4 = inf["class_maxspan"][4], inf["class_bucket_shift"][4]
    room = (1 << 15) - 256 - 1000
    past = (room - 2 * (m1 - 1) - 2 * (1 << k1)) // 2 + 1          # the smallest |shift| class 1's bound refuses
    assert m1 == 4096 and 1000 + 2 * past + m4 + 2 * (1 << k4) <= (1 << 15) - 256
    for shift in (past, -past):
        _check(ctx, data, "fb", rg, 8, shift=shift, ss=True)
    _check(ctx, data, "fb", rg, 2, shift=past - 1, ss=True)


def _reduced(ctx, reads, rg, what):
    """one plan of each reduction over ranges, as the package's own entry points make them"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    import bamsignals_amd.device as dev
    prm = make_params(_lib.MODE_PROFILE, ss=True)
    a = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
    plan = {"sum": lambda: dev.SumPlan(*a, prm),
            "xcorr": lambda: dev.XcorrPlan(*a, prm, 200),
            "hist": lambda: dev.HistPlan(*a, prm, 50),
            "summary": lambda: dev.SummaryPlan(*a, prm, [1, 2, 5]),
            "scaled": lambda: dev.ScaledPlan(*a, prm, 20)}[what]()
    try:
        return plan.run_host(), plan.stats()
    finally:
        plan.close()


def _reduced_expected(d, rg, what):
    """what _reduced's plan must give: the oracle's per-base, strand-split 5' ends of the ranges, reduced in numpy by the
    reduction's own expected side (tests/*_expected.py; the sum over ranges is the cells' sum, range by range)"""
    import crosscorr_expected as xe
    import depthhist_expected as de
    import scaled_expected as sc
    import summary_expected as se
    if what == "sum":
        return d.oracle("reduced", rg, binsize=1, shift=0, ss=True).astype(np.int64).reshape(len(rg["len"]), -1).sum(axis=0)
    if what == "xcorr":
        return xe.flat(*xe.expected(d.orc, rg, 200))
    if what == "hist":
        return de.expected(d.orc, rg, "ends", True, 50)
    if what == "summary":
        return se.expected(d.orc, rg, "ends", True, [1, 2, 5])
    return sc.expected(d.orc, rg, "ends", True, 20)


@pytest.mark.parametrize("what", ["sum", "xcorr", "hist", "summary", "scaled"])
def test_reductions_take_the_columns(ctx, data, what):
    rg = _ranges(data.cols, 2000, 600, seed=17)
    got, st = _reduced(ctx, data.on, rg, what)
    got8, st8 = _reduced(ctx, data.off, rg, what)
    assert st["bytes_per_visit_short"] == 2 and st8["bytes_per_visit_short"] == 8 and st["visits_short"] > 0
    assert np.array_equal(got, got8)
    want = _reduced_expected(data, rg, what)
    assert want.any() and got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), int(np.sum(got != want))


def test_columns_after_load_and_clone(ctx, data, tmp_path, monkeypatch):
    """bsig_reads_load and bsig_reads_clone derive the columns again (they are never saved); with
    BAMSIGNALS_SHORT_HALF=0 they leave them out, and hbm_bytes is smaller by 2 bytes a class-0/1 read at least."""
    from bamsignals_amd.device import Reads
    path = str(tmp_path / "r.bsig")
    data.on.save(path, "s")
    rg = _ranges(data.cols, 2000, 1500, seed=8)
    want = data.oracle("lc", rg, shift=75, ss=True)
    n_short = data.on.info()["class_n"][0] + data.on.info()["class_n"][1]
    hbm = {}
    for switch, bpv in ((None, 2), ("0", 8)):
        if switch is not None:
            monkeypatch.setenv("BAMSIGNALS_SHORT_HALF", switch)
        for how in ("load", "clone"):
            r = Reads.load(ctx, path, "s") if how == "load" else data.on.clone(ctx)
            try:
                got, st = _run(ctx, r, rg, shift=75, ss=True)
                assert st["bytes_per_visit_short"] == bpv and st["bytes_per_visit_packed"] == 2, (how, switch)
                assert np.array_equal(got, want), (how, switch)
                hbm[how, switch] = r.info()["hbm_bytes"]
            finally:
                r.close()
    for how in ("load", "clone"):
        assert hbm[how, None] - hbm[how, "0"] >= 2 * n_short, (how, hbm)


def test_packed_half_switch_drops_the_short_columns_too(ctx, data):
    rg = _ranges(data.cols, 2000, 500, seed=21)
    with _env("BAMSIGNALS_PACKED_HALF", "0"):
        r = _make(ctx, data.cols, True)
    try:
        got, st = _run(ctx, r, rg, shift=75, ss=True)
        assert st["bytes_per_visit_short"] == 8 and st["bytes_per_visit_packed"] == 4
        assert np.array_equal(got, data.oracle("ph", rg, shift=75, ss=True))
    finally:
        r.close()


def test_a_read_outside_its_reference_keeps_its_class_on_pos_and_fm(ctx):
    """The index files a read whose pos lies outside its reference under the reference's first or last bucket: 15 bits
    of its 5' end do not say where it is, so its class gets no column -- and the other class keeps its own."""
    cols = _columns(13, 50_000)
    far = dict(rid=1, pos=int(cols["ref_len"][1]) + 70_000, span=300)           # class 1, past the reference's last unit
    at = int(cols["ref_off"][2])
    for k, v in (("rid", far["rid"]), ("pos", far["pos"]), ("end", far["pos"] + far["span"] - 1), ("flag", 16), ("mapq", 30), ("tlen", 0)):
        cols[k] = np.insert(cols[k], at, v).astype(cols[k].dtype)
    cols["ref_off"] = cols["ref_off"].copy()
    cols["ref_off"][2:] += 1
    d = _Data.__new__(_Data)
    from oracle import oracle_c
    d.cols, d.want = cols, {}
    d.orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    d.on, d.off = _make(ctx, cols, True), _make(ctx, cols, False)
    try:
        rg = _ranges(cols, 2000, 500, seed=2)
        _check(ctx, d, "far", rg, 8, shift=75, ss=True)
    finally:
        d.close()


def test_half_kernels_keep_the_parents_registers(ctx):
    """bsig_debug_pileup_attrs(7..10) -- k_profile_half with two and one passes in flight, k_profile_multi_half, strands
    split -- no scratch, and no more VGPRs than the build before the columns had (32, 33, 39, 32)."""
    from bamsignals_amd import _lib
    fn = _lib.load().bsig_debug_pileup_attrs
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    for which, parent in ((7, 32), (8, 33), (9, 39), (10, 32)):
        regs, scratch = ctypes.c_int(0), ctypes.c_int(-1)
        assert fn(which, ctypes.byref(regs), ctypes.byref(scratch)) == 0, which
        assert scratch.value == 0, (which, scratch.value)
        assert 0 < regs.value <= parent, (which, regs.value, parent)
