"""GPU: bamCoverage with bins and strands (BSIG_MODE_COVERAGE_EX, k_coverage_bins) against the C oracle's per-base
coverage, binned and split by strand in numpy here: bin j of range i is the sum of the per-base coverage over its
bases [j*b, min((j+1)*b, w)) in range orientation; the sense row counts the reads on the range's strand ('*' = '+'),
computed by running the oracle on the reads with flag & 16 == 0 and != 0 apart."""
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
BINS = (1, 2, 7, 50, 1000, 65536)


# ---------------------------------------------------------------------------------------------------------------
# the expected values
# ---------------------------------------------------------------------------------------------------------------
def _subset(cols, mask):
    """OracleReads of the reads under `mask` (ref_off recounted per reference)."""
    from oracle import oracle_c
    ref_off = np.asarray(cols["ref_off"], dtype=np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    counts = np.bincount(rid[mask], minlength=len(ref_off) - 1)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return oracle_c.OracleReads(off, cols["pos"][mask], cols["end"][mask], cols["flag"][mask], cols["mapq"][mask],
                                cols["tlen"][mask])


def _per_base(cols, ranges, mask, **kw):
    from oracle import oracle_c
    out, off = oracle_c.coverage_core(_subset(cols, mask), ranges, **kw)
    return [out[off[i]:off[i + 1]].astype(np.int64) for i in range(len(off) - 1)]


def _binned(v, b):
    return np.add.reduceat(v, np.arange(0, len(v), b)) if len(v) else np.zeros(0, np.int64)


class Expected:
    """Per-base oracle coverage (all reads, forward reads, reverse reads) for one set of call parameters."""

    def __init__(self, cols, ranges, **kw):
        fwd = (np.asarray(cols["flag"]) & 16) == 0
        self.strand = np.asarray(ranges["strand"])
        self.all = _per_base(cols, ranges, np.ones(len(fwd), bool), **kw)
        self.fwd = _per_base(cols, ranges, fwd, **kw)
        self.rev = _per_base(cols, ranges, ~fwd, **kw)
        for a, f, r in zip(self.all, self.fwd, self.rev):
            assert np.array_equal(a, f + r)

    def get(self, b, ss):
        if not ss:
            return [_binned(v, b) for v in self.all]
        out = []
        for i, (f, r) in enumerate(zip(self.fwd, self.rev)):
            sense, anti = (r, f) if self.strand[i] < 0 else (f, r)
            out.append(np.stack([_binned(sense, b), _binned(anti, b)]))
        return out

    def flat(self, b, ss):
        parts = [m.T.reshape(-1) if ss else m for m in self.get(b, ss)]
        return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), k


# ---------------------------------------------------------------------------------------------------------------
# the reference's fixture BAM through the file-level calls
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(fixture_reads, fixture_regions):
    """The fixture's regions plus '*' ranges, a zero-width one and widths that are no multiple of any bin."""
    from bamsignals_amd import GRanges
    fx = fixture_reads
    reg, _ = fixture_regions
    names = [str(s) for s in fx["ref_names"]]
    chrom = list(reg["chrom"]) + [names[0], names[1], names[2], names[0], names[1]]
    start = list(reg["start"]) + [1, 2000, 700, 3001, 1]
    width = list(reg["width"]) + [int(fx["ref_len"][0]), 1333, 0, 7237, int(fx["ref_len"][1])]     # (whole references)
    strand = list(reg["strand"]) + ["*", "*", "-", "-", "*"]
    gr = GRanges(chrom, start, width=width, strand=strand)
    ranges = dict(rid=np.asarray([names.index(c) for c in chrom], np.int32), loc=np.asarray(start, np.int32) - 1,
                  len=np.asarray(width, np.int32), strand=np.asarray([{"+": 1, "-": -1}.get(s, 0) for s in strand], np.int32))
    cols = dict(ref_off=fx["ref_off"], pos=fx["bam_pos"], end=fx["bam_end"], flag=fx["bam_flag"], mapq=fx["bam_mapq"],
                tlen=fx["bam_tlen"])
    return gr, ranges, cols


@pytest.fixture(params=["all", "regions"], scope="module")
def decode_mode(request):
    """whole-file decode (cached in HBM) and index-driven region decode must agree"""
    from bamsignals_amd import _lib
    old = os.environ.get("BAMSIGNALS_DECODE")
    os.environ["BAMSIGNALS_DECODE"] = request.param
    _lib.load().bsig_cache_clear()
    yield request.param
    if old is None:
        os.environ.pop("BAMSIGNALS_DECODE", None)
    else:
        os.environ["BAMSIGNALS_DECODE"] = old
    _lib.load().bsig_cache_clear()


def _call_args(pe, mapqual=0, tlenFilter=None, filteredFlag=-1):
    """bamCoverage's arguments -> the oracle's (R/wrappers.R:154-173)"""
    from bamsignals_amd.wrappers import flagMask, tlenFilter as tf
    return dict(tlen_filter=tf(tlenFilter, pe), mapqual=mapqual, requiredF=flagMask(pe), filteredF=filteredFlag,
                tspan=pe == "extend")


@pytest.mark.filterwarnings("ignore:some ranges' widths")
@pytest.mark.parametrize("pe", ["ignore", "extend"])
def test_bins_and_strands_on_the_fixture(fixture, decode_mode, pe):
    from bamsignals_amd import bamCoverage
    gr, ranges, cols = fixture
    exp = Expected(cols, ranges, **_call_args(pe))
    base = bamCoverage(BAM, gr, paired_end=pe, verbose=False)          # today's per-base call
    _same(base.as_list(), exp.get(1, False))
    for b in BINS:
        flat = bamCoverage(BAM, gr, paired_end=pe, binsize=b, verbose=False)
        assert not flat.ss
        _same(flat.as_list(), exp.get(b, False))
        # bin = the sum of today's per-base coverage over its bases
        for v, w in zip(flat.as_list(), base.as_list()):
            assert np.array_equal(v, _binned(w.astype(np.int64), b))
        split = bamCoverage(BAM, gr, paired_end=pe, binsize=b, ss=True, verbose=False)
        assert split.ss
        _same(split.as_list(), exp.get(b, True))
        for m, v in zip(split.as_list(), flat.as_list()):
            assert m.shape == (2, len(v)) and np.array_equal(m[0] + m[1], v)


@pytest.mark.filterwarnings("ignore:some ranges' widths")
def test_filters_and_both_core_entry_points(fixture, decode_mode):
    from bamsignals_amd import bamCoverage
    from bamsignals_amd.wrappers import coverage_core, coverage_core_into
    gr, ranges, cols = fixture
    for pe, kw in (("ignore", dict(mapqual=30)), ("extend", dict(tlenFilter=(50, 200))), ("ignore", dict(filteredFlag=1024)),
                   ("extend", dict(mapqual=10, filteredFlag=1024, tlenFilter=(0, 300)))):
        a = _call_args(pe, **kw)
        exp = Expected(cols, ranges, **a)
        for b, ss in ((1, True), (7, False), (50, True), (1000, True)):
            _same(bamCoverage(BAM, gr, paired_end=pe, binsize=b, ss=ss, verbose=False, **kw).as_list(), exp.get(b, ss))
            core = dict(mapqual=a["mapqual"], requiredF=a["requiredF"], filteredF=a["filteredF"], tspan=a["tspan"],
                        binsize=b, ss=ss)
            _same(coverage_core(BAM, gr, a["tlen_filter"], **core), exp.get(b, ss))
            _same(coverage_core_into(BAM, gr, a["tlen_filter"], **core), exp.get(b, ss))


# ---------------------------------------------------------------------------------------------------------------
# the plan API on seeded synthetic reads
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth():
    """1e6 reads with every CIGAR of synth.py (2,100-bp spans with an N included: wider than a bin and than a 4-cell
    tile of 50-bp bins), a 5-kb tiling of both references with mixed strands and one whole-chromosome range."""
    from bamsignals_amd.device import Context, Reads
    from bamsignals_amd.synth import synth_reads, tile_ranges
    cols = synth_reads(1_000_000, [3_000_000, 1_200_017], seed=71)
    rg = tile_ranges(cols["ref_len"], 5003)
    rg["strand"] = np.asarray([1, -1, 0], np.int32)[np.arange(len(rg["rid"])) % 3]
    whole = dict(rid=np.asarray([1], np.int32), loc=np.asarray([0], np.int32),
                 len=np.asarray([cols["ref_len"][1]], np.int32), strand=np.asarray([-1], np.int32))
    rg = {k: np.concatenate([rg[k], whole[k]]) for k in rg}
    ctx = Context(0)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                  cigar_off=cols["cigar_off"], cigar=cols["cigar"])
    exp = Expected(cols, rg)
    yield ctx, reads, rg, exp
    reads.close()
    ctx.close()


def _plan_result(synth, b, ss, **kw):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, reads, rg, _ = synth
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE_EX, binsize=b, ss=ss, **kw))
    try:
        got = plan.run_host()
        assert not plan.overflowed()
        stats = plan.stats()
        again = plan.run_host()                 # a second run takes the form for resolved windows
        assert np.array_equal(got, again)
        return got, stats
    finally:
        plan.close()


@pytest.mark.parametrize("b", [1, 50, 1000])
@pytest.mark.parametrize("ss", [False, True])
def test_plan_tiles_and_threads(synth, b, ss):
    want = synth[3].flat(b, ss)
    for tile_cells in (0, 4, 64, 1000):
        for threads in (64, 128, 256):
            got, stats = _plan_result(synth, b, ss, tile_cells=tile_cells, threads=threads)
            assert np.array_equal(got, want), (tile_cells, threads)
    assert stats["cells"] == len(want) and stats["algorithmic_bytes"] >= 4 * stats["cells"]


def test_plan_mode_2_ignores_bins_and_strands(synth):
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Plan, make_params
    ctx, reads, rg, exp = synth
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE, binsize=50, ss=True))
    assert np.array_equal(plan.run_host(), exp.flat(1, False))
    plan.close()
    for bad in (0, 65537):
        with pytest.raises(_lib.BsigError) as e:
            Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE_EX, binsize=bad))
        assert e.value.code_name == "BSIG_ERR_ARG"


@pytest.mark.parametrize("b,ss", [(1, True), (50, False), (50, True), (65536, True)])
def test_heavy_slices(synth, b, ss, monkeypatch):
    """Nearly every tile cut into slices that add with global atomics: the same result, and no false overflow."""
    monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", "64")
    got, stats = _plan_result(synth, b, ss)
    assert stats["heavy_tiles"] > 0
    assert np.array_equal(got, synth[3].flat(b, ss))


# ---------------------------------------------------------------------------------------------------------------
# no wrapped value, ever
# ---------------------------------------------------------------------------------------------------------------
def _deep_bin(n_reads, heavy=None, monkeypatch=None):
    """n_reads reads that each cover the whole 65,536-bp bin [65536, 131072) of one range (half of them reverse)."""
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, Plan, Reads, make_params
    if heavy:
        monkeypatch.setenv("BAMSIGNALS_HEAVY_READS", str(heavy))
    ref_len = np.asarray([400_000], np.int64)
    pos = np.full(n_reads, 65536, np.int32)
    end = pos + 65535
    flag = np.where(np.arange(n_reads) % 2 == 0, 0, 16).astype(np.uint16)
    ctx = Context(0)
    reads = Reads(ctx, ref_len, np.asarray([0, n_reads], np.int64), pos, flag, np.full(n_reads, 60, np.uint8),
                  np.zeros(n_reads, np.int32), end=end)
    out = {}
    try:
        for ss in (False, True):
            plan = Plan(ctx, reads, [0], [0], [262_144], [1], make_params(_lib.MODE_COVERAGE_EX, binsize=65536, ss=ss))
            try:
                out[ss] = plan.run_host()
            finally:
                plan.close()
    finally:
        reads.close()
        ctx.close()
    return out


def test_a_bin_just_below_the_ceiling():
    got = _deep_bin(32_000)
    assert got[False].tolist() == [0, 2_097_152_000, 0, 0]
    assert got[True].tolist() == [0, 0, 1_048_576_000, 1_048_576_000, 0, 0, 0, 0]


def test_a_bin_just_below_the_ceiling_in_slices(monkeypatch):
    got = _deep_bin(32_000, heavy=64, monkeypatch=monkeypatch)
    assert got[False].tolist() == [0, 2_097_152_000, 0, 0]


def test_a_bin_past_the_ceiling_fails():
    from bamsignals_amd import _lib
    with pytest.raises(_lib.BsigError, match="exceeds 2"):
        _deep_bin(40_000)


def test_overflow_flag_after_an_asynchronous_run():
    import torch
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, Plan, Reads, make_params
    n = 40_000
    ctx = Context(0)
    pos = np.full(n, 65536, np.int32)
    reads = Reads(ctx, np.asarray([400_000], np.int64), np.asarray([0, n], np.int64), pos, np.zeros(n, np.uint16),
                  np.full(n, 60, np.uint8), np.zeros(n, np.int32), end=pos + 65535)
    try:
        plan = Plan(ctx, reads, [0, 0], [0, 0], [262_144, 131_072], [1, -1], make_params(_lib.MODE_COVERAGE_EX, binsize=65536))
        buf = torch.zeros(plan.cells, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        plan.run_device(buf.data_ptr())
        assert plan.overflowed()
        # the flag speaks of the last run: a plan over ranges that stay below the ceiling does not raise it
        ok = Plan(ctx, reads, [0], [300_000], [65_536], [1], make_params(_lib.MODE_COVERAGE_EX, binsize=65536, ss=True))
        assert not ok.overflowed()
        assert ok.run_host().tolist() == [0, 0]
        ok.close()
        plan.close()
    finally:
        reads.close()
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# several GPU slots in one process, and one process per rank
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:some ranges' widths")
@pytest.mark.parametrize("gather", ["xgmi", "direct", "pcie", "blocks"])
def test_multi_slot_routes(fixture, gather, monkeypatch):
    from bamsignals_amd import _lib, bamCoverage
    from bamsignals_amd.wrappers import coverage_core_into
    gr, ranges, cols = fixture
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    cases = ((50, True, "extend"), (7, False, "ignore"), (1, True, "ignore"), (1000, True, "extend"))
    _lib.load().bsig_cache_clear()
    try:
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0")
        single = {c: bamCoverage(BAM, gr, binsize=c[0], ss=c[1], paired_end=c[2], verbose=False).as_list() for c in cases}
        monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0,0,0")
        monkeypatch.setenv("BAMSIGNALS_GATHER", gather)
        for c in cases:
            got = bamCoverage(BAM, gr, binsize=c[0], ss=c[1], paired_end=c[2], verbose=False)
            assert "4 GPU slot(s)" in _lib.load().bsig_last_call_route().decode()
            _same(got.as_list(), single[c])
            a = _call_args(c[2])
            _same(coverage_core_into(BAM, gr, a["tlen_filter"], requiredF=a["requiredF"], tspan=a["tspan"], binsize=c[0], ss=c[1]),
                  single[c])
    finally:
        _lib.load().bsig_cache_clear()


_WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, {root!r})
    import numpy as np
    import torch.distributed as dist
    dist.init_process_group("gloo")
    from bamsignals_amd import GRanges
    from bamsignals_amd.dist import bamCoverage_sharded
    a = np.load({ranges!r})
    gr = GRanges([str(s) for s in a["chrom"]], a["start"], width=a["width"], strand=[str(s) for s in a["strand"]])
    res = bamCoverage_sharded({bam!r}, gr, binsize=50, ss=True, paired_end="extend")
    if dist.get_rank() == 0:
        assert res.ss
        np.savez({out!r}, *res.as_list())
    else:
        assert res is None
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
    from bamsignals_amd import bamCoverage
    gr, ranges, cols = fixture
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
    got = [z[f"arr_{i}"] for i in range(len(z.files))]
    want = bamCoverage(BAM, gr, binsize=50, ss=True, paired_end="extend", verbose=False).as_list()
    _same(got, want)
    _same(got, Expected(cols, ranges, **_call_args("extend")).get(50, True))
