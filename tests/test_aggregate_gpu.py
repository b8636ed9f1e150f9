"""GPU: sums over ranges of one width (bsig_plan_create_sum, k_sum_tiles) against the C oracle per range, summed in
int64.  Coverage with strands splits the reads by strand as test_coverage_binned_gpu.py does: the sense row counts the
reads on the range's strand ('*' = '+')."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAM = os.path.join(GOLDEN, "randomBam.bam")
REF_LEN = [2_000_000, 700_017]


# ---------------------------------------------------------------------------------------------------------------
# the expected values
# ---------------------------------------------------------------------------------------------------------------
def _oracle_reads(cols, mask=None):
    from oracle import oracle_c
    if mask is None:
        mask = np.ones(len(cols["pos"]), bool)
    ref_off = np.asarray(cols["ref_off"], dtype=np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    off = np.concatenate([[0], np.cumsum(np.bincount(rid[mask], minlength=len(ref_off) - 1))]).astype(np.int64)
    return oracle_c.OracleReads(off, cols["pos"][mask], cols["end"][mask], cols["flag"][mask], cols["mapq"][mask],
                                cols["tlen"][mask])


def _sum_rows(out, n, ss):
    s = out.astype(np.int64).reshape(n, -1).sum(axis=0) if n and out.size else np.zeros(0, np.int64)
    return s.reshape(-1, 2).T if ss else s


def want_profile(cols, rg, b, ss, **kw):
    from oracle import oracle_c
    out, _ = oracle_c.pileup_core(_oracle_reads(cols), rg, binsize=b, ss=ss, **kw)
    return _sum_rows(out, len(rg["len"]), ss)


def _binned(v, b):
    return np.add.reduceat(v, np.arange(0, v.shape[-1], b), axis=-1)


def want_coverage(cols, rg, b, ss, **kw):
    """per-base oracle coverage (all reads, or forward and reverse reads apart), binned per range, summed"""
    from oracle import oracle_c
    n, w = len(rg["len"]), int(rg["len"][0]) if len(rg["len"]) else 0
    if n == 0 or w == 0:
        return np.zeros((2, 0) if ss else (0,), np.int64)
    per = lambda m: oracle_c.coverage_core(_oracle_reads(cols, m), rg, **kw)[0].astype(np.int64).reshape(n, w)  # noqa: E731
    if not ss:
        return _binned(per(None), b).sum(axis=0)
    fwd = (np.asarray(cols["flag"]) & 16) == 0
    f, r = per(fwd), per(~fwd)
    neg = (np.asarray(rg["strand"]) < 0)[:, None]
    sense, anti = np.where(neg, r, f), np.where(neg, f, r)
    return np.stack([_binned(sense, b).sum(axis=0), _binned(anti, b).sum(axis=0)])


# ---------------------------------------------------------------------------------------------------------------
# the plan API on seeded synthetic reads
# ---------------------------------------------------------------------------------------------------------------
def _reads(ctx, cols):
    from bamsignals_amd.device import Reads
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                 cigar_off=cols["cigar_off"], cigar=cols["cigar"])


@pytest.fixture(scope="module")
def synth():
    """single-end and paired reads on two references, resident on GPU 0"""
    from bamsignals_amd.device import Context
    from bamsignals_amd.synth import synth_reads
    from oracle import oracle_c
    ctx = Context(0)
    out = {}
    for paired in (False, True):
        cols = synth_reads(400_000, REF_LEN, seed=91 + paired, paired=paired)
        cols["end"] = oracle_c.cigar_end(cols["pos"], cols["flag"], cols["cigar_off"], cols["cigar"])
        out[paired] = (cols, _reads(ctx, cols))
    yield ctx, out
    for _, r in out.values():
        r.close()
    ctx.close()


def _ranges(n, w, seed):
    from bamsignals_amd.synth import synth_ranges
    return synth_ranges(n, w, REF_LEN, seed=seed)


def _run(ctx, reads, rg, params, runs=3):
    """the sum of a plan's first run (fused lookups) and of later ones (windows kept), which must agree"""
    from bamsignals_amd.device import SumPlan
    plan = SumPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], params)
    try:
        got = [plan.run_host() for _ in range(runs)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])
        return got[0], plan.stats()
    finally:
        plan.close()


def _shape(v, ss):
    return v.reshape(-1, 2).T if ss else v


def _profile_args(pe, tlen=(50, 500)):
    from bamsignals_amd.wrappers import flagMask
    return dict(tlen_filter=() if pe == "ignore" else tlen, requiredF=flagMask(pe), pe_mid=pe == "midpoint")


@pytest.mark.parametrize("w", [1, 100, 2048, 2049, 10_000])
def test_profile_grid(synth, w):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    ctx, data = synth
    rg = _ranges(120 if w < 10_000 else 40, w, seed=w)
    for paired in (False, True):
        cols, reads = data[paired]
        for pe in (("filter", "midpoint") if paired else ("ignore",)):
            a = _profile_args(pe)
            for shift in (0, 75, -75, 70_000):
                for b in (1, 7, 50, 2000):
                    for ss in (False, True):
                        want = want_profile(cols, rg, b, ss, shift=shift, **a)
                        got, st = _run(ctx, reads, rg, make_params(_lib.MODE_PROFILE, binsize=b, shift=shift, ss=ss, **a), runs=2)
                        assert got.dtype == np.int64 and st["cells"] == got.size
                        assert np.array_equal(_shape(got, ss), want), (paired, pe, shift, b, ss)


@pytest.mark.parametrize("w", [1, 100, 2048, 2049, 10_000])
def test_coverage_grid(synth, w):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    from bamsignals_amd.wrappers import flagMask
    ctx, data = synth
    rg = _ranges(120 if w < 10_000 else 40, w, seed=7 * w)
    for paired in (False, True):
        cols, reads = data[paired]
        for pe in (("extend", "filter") if paired else ("ignore",)):
            a = dict(tlen_filter=() if pe == "ignore" else (50, 500), requiredF=flagMask(pe), tspan=pe == "extend")
            for b in (1, 7, 50, 2000):
                for ss in (False, True):
                    want = want_coverage(cols, rg, b, ss, **a)
                    got, _ = _run(ctx, reads, rg, make_params(_lib.MODE_COVERAGE_EX, binsize=b, ss=ss, **a), runs=2)
                    assert np.array_equal(_shape(got, ss), want), (paired, pe, b, ss)
            # mode 2: bins and strands ignored
            got, _ = _run(ctx, reads, rg, make_params(_lib.MODE_COVERAGE, binsize=50, ss=True, **a), runs=1)
            assert np.array_equal(got, want_coverage(cols, rg, 1, False, **a))


def test_filters_and_threads(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    ctx, data = synth
    cols, reads = data[False]
    rg = _ranges(200, 2049, seed=5)
    for kw in (dict(mapqual=20), dict(filteredF=1024), dict(mapqual=30, filteredF=1024)):
        for threads in (64, 128, 256):
            for b, ss in ((1, False), (1, True), (50, True)):
                got, _ = _run(ctx, reads, rg, make_params(_lib.MODE_PROFILE, binsize=b, ss=ss, threads=threads, **kw))
                assert np.array_equal(_shape(got, ss), want_profile(cols, rg, b, ss, **kw)), (kw, threads, b, ss)
                got, _ = _run(ctx, reads, rg, make_params(_lib.MODE_COVERAGE_EX, binsize=b, ss=ss, threads=threads, **kw))
                assert np.array_equal(_shape(got, ss), want_coverage(cols, rg, b, ss, **kw)), (kw, threads, b, ss)


@pytest.mark.parametrize("env", [{}, {"BAMSIGNALS_PACKED_HALF": "0"}, {"BAMSIGNALS_PACK": "0"}])
def test_packed_forms(synth, env, monkeypatch):
    """the half form (on by default for per-base profiles), the 4-byte words, no packed class: one answer"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    ctx, data = synth
    cols = data[False][0]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads = _reads(ctx, cols)
    try:
        rg = _ranges(300, 2048, seed=11)
        for b, ss in ((1, False), (1, True), (7, True)):
            got, st = _run(ctx, reads, rg, make_params(_lib.MODE_PROFILE, binsize=b, ss=ss))
            if not env:
                assert st["bytes_per_visit_packed"] == 2        # the sum kernel took the 16-bit column
            assert np.array_equal(_shape(got, ss), want_profile(cols, rg, b, ss))
    finally:
        reads.close()


def test_heavy_slices(synth, monkeypatch):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    ctx, data = synth
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    cols, reads = data[False]
    rg = _ranges(150, 2049, seed=3)
    for mode, b, ss in ((_lib.MODE_PROFILE, 1, True), (_lib.MODE_PROFILE, 50, False), (_lib.MODE_COVERAGE_EX, 1, False),
                        (_lib.MODE_COVERAGE_EX, 7, True)):
        got, st = _run(ctx, reads, rg, make_params(mode, binsize=b, ss=ss))
        assert st["heavy_tiles"] > 0
        want = want_profile(cols, rg, b, ss) if mode == _lib.MODE_PROFILE else want_coverage(cols, rg, b, ss)
        assert np.array_equal(_shape(got, ss), want), (mode, b, ss)


def _pile(ctx, n_reads, at=50_000, forward=False):
    """n_reads 40-bp reads starting at one base, every other one reverse (or all forward)"""
    from bamsignals_amd.device import Reads
    pos = np.full(n_reads, at, np.int32)
    flag = np.where((np.arange(n_reads) % 2 == 0) | forward, 0, 16).astype(np.uint16)
    cols = dict(ref_len=np.asarray([200_000], np.int64), ref_off=np.asarray([0, n_reads], np.int64), pos=pos, end=pos + 39,
                flag=flag, mapq=np.full(n_reads, 60, np.uint8), tlen=np.zeros(n_reads, np.int32))
    return cols, Reads(ctx, cols["ref_len"], cols["ref_off"], pos, flag, cols["mapq"], cols["tlen"], end=cols["end"])


@pytest.mark.parametrize("n_reads", [32_766, 32_767, 32_768, 32_769])
def test_piles_on_one_base(synth, n_reads):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    ctx = synth[0]
    cols, reads = _pile(ctx, n_reads)
    try:
        rg = dict(rid=np.zeros(6, np.int32), loc=np.asarray([49_000, 49_990, 49_500, 49_960, 48_000, 49_999], np.int32),
                  len=np.full(6, 3000, np.int32), strand=np.asarray([1, -1, 0, 1, -1, 0], np.int32))
        for mode, b, ss in ((_lib.MODE_PROFILE, 1, True), (_lib.MODE_PROFILE, 7, False), (_lib.MODE_COVERAGE_EX, 1, True),
                            (_lib.MODE_COVERAGE, 1, False), (_lib.MODE_COVERAGE_EX, 50, False)):
            got, st = _run(ctx, reads, rg, make_params(mode, binsize=b, ss=ss))
            want = want_profile(cols, rg, b, ss) if mode == _lib.MODE_PROFILE else want_coverage(cols, rg, b, ss)
            assert np.array_equal(_shape(got, ss), want), (mode, b, ss)
            heavy_at = 32_768 if mode == _lib.MODE_PROFILE else 32_767
            assert (st["heavy_tiles"] > 0) == (n_reads > heavy_at)
    finally:
        reads.close()


def test_past_2_to_the_32(synth):
    """140,000 identical ranges (more than 65,536 tiles of one c0) over a pile of 32,767 reads: cells above 2^32"""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import make_params
    ctx = synth[0]
    cols, reads = _pile(ctx, 32_767, forward=True)
    try:
        n = 140_000
        one = dict(rid=np.zeros(1, np.int32), loc=np.asarray([49_990], np.int32), len=np.asarray([64], np.int32),
                   strand=np.asarray([1], np.int32))
        rg = {k: np.repeat(v, n) for k, v in one.items()}
        for mode, ss in ((_lib.MODE_PROFILE, False), (_lib.MODE_PROFILE, True), (_lib.MODE_COVERAGE_EX, False)):
            got, st = _run(ctx, reads, rg, make_params(mode, ss=ss), runs=2)
            want = (want_profile(cols, one, 1, ss) if mode == _lib.MODE_PROFILE else want_coverage(cols, one, 1, ss)) * n
            assert st["n_items"] == n
            assert np.array_equal(_shape(got, ss), want) and got.max() > 2 ** 32, (mode, ss)
    finally:
        reads.close()


def test_errors_and_edges(synth):
    import ctypes as C
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, SumPlan, make_params
    ctx, data = synth
    reads = data[False][1]
    lib = _lib.load()
    with pytest.raises(_lib.BsigError, match="all signals must have the same length") as e:
        SumPlan(ctx, reads, [0, 0], [10, 500], [100, 101], [1, 1], make_params(_lib.MODE_PROFILE))
    assert e.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError) as e:
        SumPlan(ctx, reads, [0], [10], [100], [1], make_params(_lib.MODE_COUNT, binsize=-1))
    assert e.value.code_name == "BSIG_ERR_ARG"
    # a plan of each kind run the other way
    sp = SumPlan(ctx, reads, [0], [10], [100], [1], make_params(_lib.MODE_PROFILE))
    pp = Plan(ctx, reads, [0], [10], [100], [1], make_params(_lib.MODE_PROFILE))
    buf32, buf64 = np.zeros(100, np.int32), np.zeros(100, np.int64)
    assert lib.bsig_plan_run_host(sp._h, buf32.ctypes.data_as(C.c_void_p)) == -1
    assert lib.bsig_plan_run_sum_host(pp._h, buf64.ctypes.data_as(C.c_void_p)) == -1
    sp.close()
    pp.close()
    # an empty set, and ranges of width 0
    for rg in (dict(rid=[], loc=[], len=[], strand=[]), dict(rid=[0, 1], loc=[5, 9], len=[0, 0], strand=[1, -1])):
        for ss in (False, True):
            got, st = _run(ctx, reads, rg, make_params(_lib.MODE_PROFILE, ss=ss), runs=1)
            assert got.shape == (0,) and st["cells"] == 0


# ---------------------------------------------------------------------------------------------------------------
# the file-level calls on the reference's fixture BAM
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(fixture_reads):
    """fixed-width ranges over the fixture's references, mixed strands"""
    from bamsignals_amd import GRanges
    fx = fixture_reads
    names = [str(s) for s in fx["ref_names"]]
    rng = np.random.default_rng(17)
    n, w = 60, 1500
    rid = rng.integers(0, len(names), n).astype(np.int32)
    loc = np.asarray([rng.integers(0, int(fx["ref_len"][r]) - w) for r in rid], np.int32)
    strand = np.asarray([1, -1, 0], np.int32)[rng.integers(0, 3, n)]
    gr = GRanges([names[r] for r in rid], loc + 1, width=np.full(n, w), strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in strand])
    rg = dict(rid=rid, loc=loc, len=np.full(n, w, np.int32), strand=strand)
    cols = dict(ref_off=fx["ref_off"], pos=fx["bam_pos"], end=fx["bam_end"], flag=fx["bam_flag"], mapq=fx["bam_mapq"],
                tlen=fx["bam_tlen"])
    return gr, rg, cols


@pytest.fixture(params=["all", "regions"])
def decode_mode(request, monkeypatch):
    from bamsignals_amd import _lib
    monkeypatch.setenv("BAMSIGNALS_DECODE", request.param)
    _lib.load().bsig_cache_clear()
    yield request.param
    _lib.load().bsig_cache_clear()


@pytest.mark.filterwarnings("ignore:some ranges' widths")
def test_file_level(fixture, decode_mode):
    from bamsignals_amd import bamCoverage, bamProfile
    from bamsignals_amd.wrappers import flagMask, tlenFilter
    gr, rg, cols = fixture
    for b, ss in ((1, False), (1, True), (7, True), (50, False)):
        for pe in ("ignore", "midpoint"):
            a = dict(tlen_filter=tlenFilter(None, pe), requiredF=flagMask(pe), pe_mid=pe == "midpoint")
            got = bamProfile(BAM, gr, binsize=b, ss=ss, shift=3, paired_end=pe, verbose=False, aggregate=True)
            assert got.dtype == np.int64
            assert np.array_equal(got, want_profile(cols, rg, b, ss, shift=3, **a)), (b, ss, pe)
            sig = bamProfile(BAM, gr, binsize=b, ss=ss, shift=3, paired_end=pe, verbose=False)
            assert np.array_equal(got, np.asarray(sig.alignSignals(), np.int64).sum(axis=-1))
        for pe in ("ignore", "extend"):
            a = dict(tlen_filter=tlenFilter(None, pe), requiredF=flagMask(pe), tspan=pe == "extend")
            got = bamCoverage(BAM, gr, binsize=b, ss=ss, paired_end=pe, verbose=False, aggregate=True)
            assert np.array_equal(got, want_coverage(cols, rg, b, ss, **a)), (b, ss, pe)


@pytest.mark.filterwarnings("ignore:some ranges' widths")
def test_four_slots_equal_one(fixture, monkeypatch):
    from bamsignals_amd import _lib, bamCoverage, bamProfile
    gr = fixture[0]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    try:
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
        one = (bamProfile(BAM, gr, binsize=7, ss=True, verbose=False, aggregate=True),
               bamCoverage(BAM, gr, binsize=50, ss=True, paired_end="extend", verbose=False, aggregate=True))
        assert "sum" in _lib.load().bsig_last_call_route().decode()
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
        four = (bamProfile(BAM, gr, binsize=7, ss=True, verbose=False, aggregate=True),
                bamCoverage(BAM, gr, binsize=50, ss=True, paired_end="extend", verbose=False, aggregate=True))
        route = _lib.load().bsig_last_call_route().decode()
        assert "4 GPU slot(s)" in route and "sum" in route
        for a, b in zip(one, four):
            assert np.array_equal(a, b)
    finally:
        _lib.load().bsig_cache_clear()


_WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, {root!r})
    import numpy as np
    import torch.distributed as dist
    dist.init_process_group("gloo")
    from bamsignals_amd import GRanges
    from bamsignals_amd.dist import bamCoverage_sharded, bamProfile_sharded
    a = np.load({ranges!r})
    gr = GRanges([str(s) for s in a["chrom"]], a["start"], width=a["width"], strand=[str(s) for s in a["strand"]])
    p = bamProfile_sharded({bam!r}, gr, binsize=7, ss=True, aggregate=True)
    c = bamCoverage_sharded({bam!r}, gr, binsize=50, ss=True, paired_end="extend", aggregate=True)
    if dist.get_rank() == 0:
        np.savez({out!r}, p=p, c=c)
    else:
        assert p is None and c is None
    dist.destroy_process_group()
""")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.filterwarnings("ignore:some ranges' widths")
@pytest.mark.timeout(600)
def test_sharded_over_two_ranks(fixture, tmp_path):
    from bamsignals_amd import bamCoverage, bamProfile
    gr = fixture[0]
    rfile, out = str(tmp_path / "ranges.npz"), str(tmp_path / "out.npz")
    np.savez(rfile, chrom=np.asarray(gr.seqnames), start=gr.start, width=gr.width, strand=np.asarray(gr.strand))
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, ranges=rfile, bam=BAM, out=out))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BAMSIGNALS_DEVICES", "BAMSIGNALS_DEVICE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(script)]
    run = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=560, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["p"], bamProfile(BAM, gr, binsize=7, ss=True, verbose=False, aggregate=True))
    assert np.array_equal(z["c"], bamCoverage(BAM, gr, binsize=50, ss=True, paired_end="extend", verbose=False, aggregate=True))
