"""GPU: spliced reads (rows = aligned blocks) at handle level and bamCoverage(splice=True) / bamViews(splice=True) at file
level, against tests/spliced_expected.py: the numpy restatement of the semantics and the existing oracle applied to the block
columns.  All results are integers and compared exactly."""
import os

import numpy as np
import pytest

import spliced_expected as sx
from bamsignals_amd import GRanges, _lib, bamCoverage, bamViews
from bamsignals_amd.bamio import BamFile, write_columns_as_bam
from bamsignals_amd.device import (CappedPlan, Context, FragPlan, Plan, Reads, SumPlan, VplotPlan, XcorrPlan, make_params)
from bamsignals_amd.synth import synth_reads, tile_ranges
from bamsignals_amd.wrappers import last_call_route, last_call_timing

pytestmark = pytest.mark.gpu

I32 = np.int32


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def decks():
    """name -> (CIGAR columns, the restated block columns): computed once, shared, left unchanged"""
    out = {}
    for name, cols in (("hand", sx.hand_deck()), ("random", sx.random_deck()),
                       ("synth", synth_reads(20000, [1_000_000, 400_000], seed=11))):
        out[name] = (cols, sx.blocks(cols))
    return out


def upload(ctx, cols, spliced=True):
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                 cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=spliced)


def ranges_for(cols, width):
    """a tiling, '-' ranges among them"""
    rg = tile_ranges(cols["ref_len"], width)
    rg["strand"] = (np.arange(len(rg["rid"])) % 3 - 1).astype(I32)
    return rg


# ---- handle level -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck", ["hand", "random", "synth"])
def test_reads_are_the_restated_blocks(ctx, decks, deck):
    cols, b = decks[deck]
    reads = upload(ctx, cols)
    assert reads.spliced and reads.info()["n_reads"] == len(b["pos"])
    plain = upload(ctx, cols, spliced=False)
    assert not plain.spliced and plain.info()["n_reads"] == len(cols["pos"])
    clone = reads.clone(ctx)
    assert clone.spliced and clone.info()["n_reads"] == len(b["pos"])
    for r in (reads, plain, clone):
        r.close()


@pytest.mark.parametrize("deck, width", [("hand", 100), ("hand", 2048), ("hand", 5000), ("random", 100), ("random", 1000),
                                         ("random", 2048), ("random", 5000), ("synth", 2048)])
def test_plain_coverage_plan(ctx, decks, deck, width):
    cols, b = decks[deck]
    if deck == "hand" and width == 100:         # (a 3-Mb reference in 100-base tiles: the stretches where the deck lives)
        rg = tile_ranges([6000, 5000, 4000], width)
        more = tile_ranges([2000], width)
        for base, rid in ((999_000, 0), (1_999_000, 0), (2_998_000, 0), (99_000, 2), (169_000, 2), (398_000, 2)):
            rg = {k: np.concatenate([rg[k], dict(more, rid=np.full_like(more["rid"], rid), loc=more["loc"] + base)[k]]) for k in rg}
        rg["strand"] = (np.arange(len(rg["rid"])) % 3 - 1).astype(I32)
    else:
        rg = ranges_for(cols, width)
    reads = upload(ctx, cols)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE))
    got = plan.run_host()
    want = sx.expected_coverage(b, rg)
    assert np.array_equal(got, want)
    assert got.sum() > 0
    plan.close()
    reads.close()


@pytest.mark.parametrize("binsize, ss", [(1, 0), (7, 1), (200, 1)])
@pytest.mark.parametrize("deck", ["hand", "random"])
def test_binned_stranded_plan(ctx, decks, deck, binsize, ss):
    cols, b = decks[deck]
    rg = ranges_for(cols, 5000)
    reads = upload(ctx, cols)
    for flt in (dict(), dict(mapqual=30, filteredF=0x400)):
        plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"],
                    make_params(_lib.MODE_COVERAGE_EX, binsize=binsize, ss=bool(ss), **flt))
        assert np.array_equal(plan.run_host(), sx.expected_coverage(b, rg, binsize=binsize, ss=bool(ss), **flt)), flt
        plan.close()
    reads.close()


def test_ranges_inside_introns_and_far_downstream(ctx, decks):
    cols, b = decks["hand"]
    # wholly inside the megabase intron (all zero); blocks whose reads start a megabase upstream; the gap past the end
    rg = dict(rid=np.asarray([0, 0, 0, 0, 2], I32), loc=np.asarray([1_200_000, 2_000_040, 2_000_000, 2_999_900, 1_200], I32),
              len=np.asarray([50_000, 30, 200, 300, 700], I32), strand=np.asarray([1, -1, 0, 1, -1], I32))
    reads = upload(ctx, cols)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE))
    got = plan.run_host()
    assert np.array_equal(got, sx.expected_coverage(b, rg))
    assert not got[:50_000].any() and got[50_000:50_030].min() >= 1
    assert not got[plan.offsets[4]:plan.offsets[5]].any(), "between the exons of the reads at chr3:1000"
    plan.close()
    reads.close()


def test_sum_runs_and_views(ctx, decks):
    import torch
    cols, b = decks["random"]
    rg = ranges_for(cols, 1000)
    reads = upload(ctx, cols)
    want = sx.expected_coverage(b, rg, binsize=10, ss=True)
    prm = make_params(_lib.MODE_COVERAGE_EX, binsize=10, ss=True)
    sp = SumPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], prm)
    assert np.array_equal(sp.run_host(), want.reshape(len(rg["rid"]), -1).astype(np.int64).sum(axis=0))
    sp.close()
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], prm)
    buf = torch.empty(max(plan.cells, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    plan.run_device(buf.data_ptr())
    ctx.sync()
    rows = want.reshape(len(rg["rid"]), -1, 2).transpose(0, 2, 1).reshape(2 * len(rg["rid"]), -1)      # segment 2 i + antisense
    enc = plan.runs()
    enc.encode(buf.data_ptr())
    seg_off, values, lengths = enc.fetch()
    for k in (0, 1, 7, len(rows) - 1):
        assert np.array_equal(np.repeat(values[seg_off[k]:seg_off[k + 1]], lengths[seg_off[k]:seg_off[k + 1]]), rows[k])
    change = sum(1 + int(np.count_nonzero(np.diff(r))) for r in rows)
    assert enc.n_runs == change
    enc.close()
    ve = plan.views()
    n = ve.encode(buf.data_ptr(), 5)
    seg_off, start, width, total, mx, summit = ve.fetch()
    edges = sum(int(np.count_nonzero(np.diff(np.concatenate([[0], (r >= 5).astype(np.int8), [0]])) == 1)) for r in rows)
    assert n == edges > 0
    assert int(total.sum()) == int(sum(r[r >= 5].sum() for r in rows))
    ve.close()
    plan.close()
    reads.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_read_counts_at_the_scan_and_sort_edges(ctx, decks, n):
    cols = sx.spliced_prefix(decks["random"][0], n)
    b = sx.blocks(cols)
    assert n == 0 or len(b["pos"]) > n
    reads = upload(ctx, cols)
    assert reads.info()["n_reads"] == len(b["pos"])
    rg = ranges_for(cols, 5000)
    plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE_EX, binsize=7, ss=True))
    assert np.array_equal(plan.run_host(), sx.expected_coverage(b, rg, binsize=7, ss=True))
    plan.close()
    reads.close()


def test_save_and_every_other_plan_refuse(ctx, decks, tmp_path):
    cols, _ = decks["random"]
    reads = upload(ctx, cols)
    rg = ranges_for(cols, 1000)
    args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])

    def refused(make, words):
        with pytest.raises(_lib.BsigError, match=words) as ei:
            make()
        assert ei.value.code_name == "BSIG_ERR_ARG"

    refused(lambda: reads.save(str(tmp_path / "x.bsig"), "s"), "spliced reads have no reads file")
    assert not os.path.exists(tmp_path / "x.bsig")
    refused(lambda: Plan(*args, make_params(_lib.MODE_PROFILE)), "spliced reads give coverage only")
    refused(lambda: Plan(*args, make_params(_lib.MODE_COUNT, binsize=-1)), "spliced reads give coverage only")
    refused(lambda: Plan(*args, make_params(_lib.MODE_COVERAGE, tspan=True, tlen_filter=(0, 1000))), "spliced reads: tspan")
    refused(lambda: Plan(*args, make_params(_lib.MODE_COVERAGE_EX, tspan=True, tlen_filter=(0, 1000))), "spliced reads: tspan")
    refused(lambda: Plan(*args, make_params(_lib.MODE_COVERAGE), frag_len=150), "spliced reads: frag_len")
    refused(lambda: SumPlan(*args, make_params(_lib.MODE_COVERAGE_EX), frag_len=150), "spliced reads: frag_len")
    refused(lambda: SumPlan(*args, make_params(_lib.MODE_PROFILE)), "spliced reads give coverage only")
    refused(lambda: Plan(*args, make_params(_lib.MODE_OVERLAP_ANY, binsize=1)), "spliced reads: bamOverlaps")
    refused(lambda: XcorrPlan(*args, make_params(_lib.MODE_PROFILE, ss=True), 100), "spliced reads: the strand cross-correlation")
    refused(lambda: FragPlan(*args, make_params(_lib.MODE_COUNT, tlen_filter=(0, 500)), 10), "spliced reads: the fragment-length histogram")
    refused(lambda: VplotPlan(*args, make_params(_lib.MODE_PROFILE, tlen_filter=(0, 500)), 10), "spliced reads: the V-plot")
    refused(lambda: CappedPlan(*args, make_params(_lib.MODE_PROFILE), 1), "spliced reads: keep_dup")
    refused(lambda: CappedPlan(*args, make_params(_lib.MODE_COVERAGE_EX), 1, 150), "spliced reads: keep_dup")
    reads.close()


# ---- file level -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    """name -> (path, CIGAR columns as the file holds them, their restated blocks, GRanges tiling, the same as range arrays)"""
    d = tmp_path_factory.mktemp("spliced")
    out = {}
    for name, cols in (("hand", sx.hand_deck()), ("random", sx.random_deck())):
        names = [f"chr{k + 1}" for k in range(len(cols["ref_len"]))]
        path = str(d / f"{name}.bam")
        write_columns_as_bam(path, names, cols)
        width = 5000
        rg = tile_ranges(cols["ref_len"], width)
        rg["strand"] = (np.arange(len(rg["rid"])) % 3 - 1).astype(I32)
        gr = GRanges([names[r] for r in rg["rid"]], rg["loc"] + 1, width=rg["len"], strand=["-+*"[s + 1] for s in rg["strand"]])
        out[name] = (path, cols, sx.blocks(cols), gr, rg)
    return out


def _flat(sig, ss):
    return np.concatenate([(np.asarray(m).T.reshape(-1) if ss else np.asarray(m)) for m in sig])


def check_file_calls(bam):
    path, cols, b, gr, rg = bam
    for binsize, ss in ((1, False), (7, True), (200, True)):
        want = sx.expected_coverage(b, rg, binsize=binsize, ss=ss)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sig = bamCoverage(path, gr, verbose=False, binsize=binsize, ss=ss, splice=True)
            assert np.array_equal(_flat(sig, ss), want), (binsize, ss)
            assert "spliced" in last_call_route()
            runs = bamCoverage(path, gr, verbose=False, binsize=binsize, ss=ss, splice=True, runs=True)
        for i in (0, 1, len(gr) - 1):
            assert np.array_equal(np.asarray(runs.decode(i)), np.asarray(sig[i]))
    # ranges of one width: the first reference's tiles
    n0 = int(np.count_nonzero(rg["rid"] == 0)) - 1
    sub = {k: v[:n0] for k, v in rg.items()}
    gr0 = GRanges(["chr1"] * n0, sub["loc"] + 1, width=sub["len"], strand=["-+*"[s + 1] for s in sub["strand"]])
    agg = bamCoverage(path, gr0, verbose=False, binsize=10, ss=True, aggregate=True, splice=True)
    want = sx.expected_coverage(b, sub, binsize=10, ss=True).reshape(n0, -1, 2).astype(np.int64).sum(axis=0).T
    assert np.array_equal(agg, want)
    v = bamViews(path, gr, 2, verbose=False, splice=True)
    per = sx.expected_coverage(b, rg)
    off = np.concatenate([[0], np.cumsum(rg["len"])])
    n_views = sum(int(np.count_nonzero(np.diff(np.concatenate([[0], (per[off[i]:off[i + 1]] >= 2).astype(np.int8), [0]])) == 1))
                  for i in range(len(gr)))
    assert v.nviews == n_views > 0
    assert int(np.asarray(v.sum).sum()) == int(per[per >= 2].sum())
    # mapqual and filteredFlag act on blocks as on reads
    sig = bamCoverage(path, gr, mapqual=30, filteredFlag=0x400, verbose=False, splice=True)
    assert np.array_equal(_flat(sig, False), sx.expected_coverage(b, rg, mapqual=30, filteredF=0x400))


@pytest.mark.parametrize("device_decode", ["require", "0"])
@pytest.mark.parametrize("decode", ["all", "regions"])
@pytest.mark.parametrize("deck", ["hand", "random"])
def test_file_level_on_every_decode_route(bams, monkeypatch, deck, decode, device_decode):
    monkeypatch.setenv("BAMSIGNALS_DECODE", decode)
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", device_decode)
    _lib.load().bsig_cache_clear()
    check_file_calls(bams[deck])
    _lib.load().bsig_cache_clear()


def test_several_chunks_inflated_on_the_gpu(tmp_path, monkeypatch):
    """a file of several 1-MB chunks (sequences pad the records): every chunk leaves its piece of the gap table"""
    cols = synth_reads(20000, [1_000_000, 400_000], seed=11)
    path = str(tmp_path / "padded.bam")
    write_columns_as_bam(path, ["chr1", "chr2"], cols, l_seq=100, seed=3)
    assert os.path.getsize(path) > 1_500_000
    monkeypatch.setenv("BAMSIGNALS_INFLATE", "gpu")
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE_CHUNK_MB", "1")
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", "require")
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    rg = tile_ranges(cols["ref_len"], 4096)
    gr = GRanges([f"chr{r + 1}" for r in rg["rid"]], rg["loc"] + 1, width=rg["len"])
    sig = bamCoverage(path, gr, verbose=False, splice=True)
    b = sx.blocks(cols)
    assert np.array_equal(_flat(sig, False), sx.expected_coverage(b, rg))
    ctx = Context(0)
    bam = BamFile(path)
    reads = Reads.from_bam(ctx, bam, spliced=True)
    assert reads.spliced and reads.info()["n_reads"] == len(b["pos"])
    part = Reads.from_bam_regions(ctx, bam, [0], [100_000], [300_000], spliced=True)
    assert part.spliced and 0 < part.info()["n_reads"] < len(b["pos"])
    for x in (reads, part, bam, ctx):
        x.close()
    _lib.load().bsig_cache_clear()


def test_one_gpu_listed_twice(bams, monkeypatch):
    monkeypatch.setenv("BAMSIGNALS_DEVICES", "0,0")
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    _lib.load().bsig_cache_clear()
    check_file_calls(bams["random"])
    assert last_call_route().startswith("2 GPU slot(s)")
    _lib.load().bsig_cache_clear()


def test_cache_keeps_plain_and_spliced_apart(bams, monkeypatch, tmp_path):
    path, cols, b, gr, rg = bams["random"]
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    monkeypatch.setenv("BAMSIGNALS_SIDECAR_DIR", str(tmp_path))
    _lib.load().bsig_cache_clear()
    plain_want = sx.expected_coverage(dict(cols, end=sx.ends(cols)), rg)
    spliced_want = sx.expected_coverage(b, rg)
    assert not np.array_equal(plain_want, spliced_want)
    first = _flat(bamCoverage(path, gr, verbose=False), False)
    assert not last_call_timing()["bam_was_resident"]
    sidecars = sorted(os.listdir(tmp_path))
    assert len(sidecars) == 1, "the plain call writes its reads file"
    second = _flat(bamCoverage(path, gr, verbose=False, splice=True), False)
    assert not last_call_timing()["bam_was_resident"] and "spliced" in last_call_route()
    third = _flat(bamCoverage(path, gr, verbose=False), False)
    assert last_call_timing()["bam_was_resident"] and "reads: resident" in last_call_route()
    fourth = _flat(bamCoverage(path, gr, verbose=False, splice=True), False)
    assert last_call_timing()["bam_was_resident"] and "spliced, resident" in last_call_route()
    assert np.array_equal(first, plain_want) and np.array_equal(third, plain_want)
    assert np.array_equal(second, spliced_want) and np.array_equal(fourth, spliced_want)
    # a plain reads file beside the BAM does not change a spliced result, and no spliced reads file appears
    _lib.load().bsig_cache_clear()
    again = _flat(bamCoverage(path, gr, verbose=False, splice=True), False)
    assert np.array_equal(again, spliced_want) and "sidecar" not in last_call_route()
    assert sorted(os.listdir(tmp_path)) == sidecars
    _lib.load().bsig_cache_clear()


def test_without_n_splice_changes_nothing(tmp_path, monkeypatch):
    cols = sx.random_deck()
    coff, cig = cols["cigar_off"], cols["cigar"]
    keep = np.flatnonzero([not np.any((cig[coff[i]:coff[i + 1]] & 0xF) == 3) for i in range(len(cols["pos"]))])
    cols = sx.take(cols, keep)
    path = str(tmp_path / "no_n.bam")
    write_columns_as_bam(path, ["chr1", "chr2", "chr3"], cols)
    rg = tile_ranges(cols["ref_len"], 2048)
    gr = GRanges([f"chr{r + 1}" for r in rg["rid"]], rg["loc"] + 1, width=rg["len"])
    _lib.load().bsig_cache_clear()
    a = bamCoverage(path, gr, verbose=False, splice=True)
    p = bamCoverage(path, gr, verbose=False)
    assert len(a) == len(p) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, p))
    assert _flat(a, False).sum() > 0
    _lib.load().bsig_cache_clear()
