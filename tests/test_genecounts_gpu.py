"""GPU: the read table of spliced reads and the gene counts at handle level (Reads.gene_counts) and at file level
(bamGeneCounts), against tests/genecounts_expected.py: the rule restated in numpy, never flattened.  All results are integers
and compared exactly; nothing is timed."""
import functools

import numpy as np
import pytest

import genecounts_expected as gx
import spliced_expected as sx
from bamsignals_amd import GeneModel, GRanges, _lib, bamCoverage, bamGeneCounts
from bamsignals_amd.bamio import BamFile, write_columns_as_bam
from bamsignals_amd.device import Context, Reads
from bamsignals_amd.synth import tile_ranges
from bamsignals_amd.wrappers import last_call_route, last_call_timing
from test_junctions_gpu import FILTERS

pytestmark = pytest.mark.gpu

NAMES = ["chr1", "chr2", "chr3", "chr4", "chr5"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def upload(ctx, cols, spliced=True):
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                 cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=spliced)


def model_of(ann, n_ref, names=None):
    f = ann.features
    return GeneModel.from_arrays(f["rid"], f["loc"], f["len"], f["strand"], ann.gene, ann.n_genes, n_ref, genes=ann.labels, seqlevels=names)


@pytest.fixture(scope="module")
def decks(ctx):
    """name -> (CIGAR columns, annotation, its model, the resident spliced set): made once, shared, left unchanged; the two
    junction decks share one set"""
    out, sets = {}, {}
    for name in gx.DECKS:
        cols, ann = gx.deck(name)
        if id(cols) not in sets:
            sets[id(cols)] = upload(ctx, cols)
        out[name] = (cols, ann, model_of(ann, len(cols["ref_len"])), sets[id(cols)])
    yield out
    for reads in sets.values():
        reads.close()
    for _, _, model, _ in out.values():
        model.close()


@functools.lru_cache(maxsize=None)
def want(deck, mode, k_filter):
    """the restatement's (counts, summary), computed once per case and shared"""
    cols, ann = gx.deck(deck)
    return gx.expected(cols, ann.features, ann.gene, ann.n_genes, strand=mode, **FILTERS[k_filter])


def same(got, exp):
    return all(np.asarray(g).dtype == np.int64 and np.asarray(g).shape == np.asarray(e).shape and np.array_equal(g, e) for g, e in zip(got, exp))


# ---- query == restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_filter", range(len(FILTERS)))
@pytest.mark.parametrize("mode", gx.MODES)
@pytest.mark.parametrize("deck", gx.DECKS)
def test_query_is_the_restatement(decks, deck, mode, k_filter):
    cols, ann, model, reads = decks[deck]
    exp = want(deck, mode, k_filter)
    got = reads.gene_counts(model, strand=mode, **FILTERS[k_filter])
    assert same(got, exp), (got[1], exp[1])
    counts, summary = got
    assert len(counts) == ann.n_genes and summary.sum() == reads.n_source_reads == len(cols["pos"]) and counts.sum() == summary[0]
    # the deck's features given twice and reversed, with the same genes
    again = model_of(ann.twice_and_reversed(), len(cols["ref_len"]))
    assert same(reads.gene_counts(again, strand=mode, **FILTERS[k_filter]), exp)
    again.close()


def test_required_flags(decks):
    """paired_end="filter" at handle level: requiredF = 66 on the deck with mate flags"""
    cols, ann, model, reads = decks["random"]
    for mode in gx.MODES:
        exp = gx.expected(cols, ann.features, ann.gene, ann.n_genes, strand=mode, requiredF=66)
        assert exp[1][3] > 3000 and same(reads.gene_counts(model, strand=mode, requiredF=66), exp)


# ---- the table with the set -------------------------------------------------------------------------------------------------
def test_clone_plain_and_refusals(ctx, decks):
    cols, ann, model, reads = decks["hand"]
    assert reads.spliced and reads.n_source_reads == len(cols["pos"]) and reads.info()["n_reads"] > 35_000 > reads.n_source_reads
    clone = reads.clone(ctx)
    assert clone.n_source_reads == reads.n_source_reads
    assert same(clone.gene_counts(model, strand="forward"), want("hand", "forward", 0))
    # 8 bytes per read and 8 per block, in the clone's own memory
    n_blocks = len(gx.read_blocks(cols)[0])
    assert clone.info()["hbm_bytes"] >= 8 * len(cols["pos"]) + 8 * n_blocks
    clone.close()
    plain = upload(ctx, cols, spliced=False)
    assert not plain.spliced and plain.n_source_reads == 0
    assert reads.info()["hbm_bytes"] - plain.info()["hbm_bytes"] >= 8 * n_blocks, "hbm_bytes grew by the table"
    with pytest.raises(_lib.BsigError, match="gene counts need spliced reads") as ei:
        plain.gene_counts(model)
    assert ei.value.code_name == "BSIG_ERR_ARG"
    plain.close()
    other = model_of(ann, len(cols["ref_len"]) + 1)
    with pytest.raises(_lib.BsigError, match="the gene model has 6 references, the reads have 5"):
        reads.gene_counts(other)
    other.close()
    with pytest.raises(ValueError, match="strand must be one of"):
        reads.gene_counts(model, strand="sense")
    with pytest.raises(TypeError, match="GeneModel"):
        reads.gene_counts(None)
    counts, summary = np.zeros(ann.n_genes, np.int64), np.zeros(5, np.int64)
    lib = _lib.load()
    assert lib.bsig_reads_gene_counts(reads._h, model._h, 0, 0, -1, 3, counts.ctypes.data, summary.ctypes.data) == -1
    assert lib.bsig_last_error().decode() == "strandedness must be 0 (unstranded), 1 (forward) or 2 (reverse): 3 given"


def test_empty_set_empty_model_and_genes_without_features(ctx, decks):
    cols, ann, model, reads = decks["hand"]
    n_ref = len(cols["ref_len"])
    none = sx.take({k: v for k, v in cols.items()}, np.zeros(0, dtype=np.int64))
    empty = upload(ctx, none)
    assert empty.spliced and empty.n_source_reads == 0
    counts, summary = empty.gene_counts(model)
    assert counts.shape == (ann.n_genes,) and not counts.any() and summary.tolist() == [0] * 5
    empty.close()
    no_genes = GeneModel.from_arrays([], [], [], [], [], 0, n_ref)
    counts, summary = reads.gene_counts(no_genes)
    assert counts.shape == (0,) and summary.tolist() == [0, 0, len(cols["pos"]) - 1, 0, 1]
    bare = GeneModel.from_arrays([], [], [], [], [], 7, n_ref)
    counts, summary = reads.gene_counts(bare, strand="reverse", mapqual=30)
    assert counts.shape == (7,) and not counts.any() and summary[0] == summary[1] == 0 and summary.sum() == len(cols["pos"])
    widthless = GeneModel.from_arrays([0, 2], [100, 1000], [0, 0], [1, -1], [0, 1], 2, n_ref)
    counts, summary = reads.gene_counts(widthless)
    assert counts.tolist() == [0, 0] and summary[0] == 0 and summary.sum() == len(cols["pos"])


# ---- both decode routes -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    """name -> (path, names, columns, annotation): the decks written as BAM files; "half": the first half of the junction deck"""
    d = tmp_path_factory.mktemp("genecounts")
    out = {}
    for name in ("junction", "random", "half"):
        cols, ann = gx.deck("junction" if name == "half" else name)
        if name == "half":
            cols = sx.take({k: v for k, v in cols.items()}, np.arange(len(cols["pos"]) // 2))
        names = NAMES[:len(cols["ref_len"])]
        path = str(d / f"{name}.bam")
        write_columns_as_bam(path, names, {k: np.array(v) for k, v in cols.items()})
        out[name] = (path, names, cols, ann)
    return out


@pytest.mark.parametrize("deck", ["junction", "random"])
def test_both_decode_routes(ctx, decks, bams, deck):
    """the read table from the CIGAR columns and from the inflated stream of the same deck agree with each other and with
    the restatement"""
    path, names, cols, ann = bams[deck]
    _, _, model, from_columns = decks[deck]
    bam = BamFile(path)
    from_stream = Reads.from_bam(ctx, bam, spliced=True)
    bam.close()
    assert from_stream.spliced and from_stream.n_source_reads == from_columns.n_source_reads == len(cols["pos"])
    for mode in gx.MODES:
        for k in range(len(FILTERS)):
            a, b = from_stream.gene_counts(model, strand=mode, **FILTERS[k]), from_columns.gene_counts(model, strand=mode, **FILTERS[k])
            assert same(a, b) and same(a, want(deck, mode, k)), (mode, k)
    from_stream.close()


# ---- file level -------------------------------------------------------------------------------------------------------------
def granges_of(ann, names):
    f = ann.features
    return GRanges([names[r] for r in f["rid"]], f["loc"].astype(np.int64) + 1, width=f["len"], strand=["-*+"[s + 1] for s in f["strand"]]), \
        [ann.labels[g] for g in ann.gene]


def test_file_level(decks, bams):
    path, names, cols, ann = bams["junction"]
    _, _, model, reads = decks["junction"]
    lib = _lib.load()
    lib.bsig_cache_clear()
    tiles = tile_ranges(cols["ref_len"], 5000)
    gr_cov = GRanges([names[r] for r in tiles["rid"]], tiles["loc"] + 1, width=tiles["len"])
    before = bamCoverage(path, gr_cov, verbose=False, splice=True)
    assert not last_call_timing()["bam_was_resident"] and "spliced" in last_call_route()
    gr, group = granges_of(ann, names)
    for mode, kw, k in (("unstranded", dict(), 0), ("forward", dict(mapqual=30, filteredFlag=0x400), 1), ("reverse", dict(), 0)):
        got = bamGeneCounts(path, gr, group, strand=mode, verbose=False, **kw)
        route = last_call_route()
        assert "gene counts" in route and last_call_timing()["bam_was_resident"] and "spliced, resident" in route, \
            "the coverage call's spliced set"
        assert got.genes == tuple(ann.labels) and same((got.counts, got.summary), want("junction", mode, k))
        assert same((got.counts, got.summary), reads.gene_counts(model, strand=mode, **FILTERS[k]))
        assert not got.counts.flags.writeable and not got.summary.flags.writeable and got.n_reads == len(cols["pos"])
    after = bamCoverage(path, gr_cov, verbose=False, splice=True)
    assert last_call_timing()["bam_was_resident"] and "spliced, resident" in last_call_route()
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(before, after))
    lib.bsig_cache_clear()
    # a cold call decodes the whole file whatever the features cover
    one = GRanges([names[0]], [1001], width=[50], strand=["+"])
    got = bamGeneCounts(path, one, ["only"], verbose=False)
    assert not last_call_timing()["bam_was_resident"] and got.n_reads == len(cols["pos"]) and got.no_feature > 12_000
    lib.bsig_cache_clear()


def test_file_level_model_on_two_files_and_pairs(bams):
    path, names, cols, ann = bams["junction"]
    half_path, _, half_cols, _ = bams["half"]
    gr, group = granges_of(ann, names)
    model = GeneModel(gr, group)
    both = bamGeneCounts([path, half_path], model, strand="forward", verbose=False)
    assert both.counts.shape == (ann.n_genes, 2) and both.summary.shape == (2, 5) and both.files == (path, half_path)
    assert same((both.counts[:, 0], both.summary[0]), want("junction", "forward", 0))
    assert same((both.counts[:, 1], both.summary[1]), gx.expected(half_cols, ann.features, ann.gene, ann.n_genes, strand="forward"))
    assert both.n_reads.tolist() == [len(cols["pos"]), len(half_cols["pos"])]
    # the features' sequences are matched by name: given in another order the model's references are other indices
    order = np.argsort(-ann.features["rid"], kind="stable")
    shuffled = bamGeneCounts(path, gr[order], [group[k] for k in order], strand="forward", verbose=False)
    assert dict(zip(shuffled.genes, shuffled.counts.tolist())) == dict(zip(both.genes, both.counts[:, 0].tolist()))
    # proper pairs by their first mate, on the deck with mate flags
    rpath, rnames, rcols, rann = bams["random"]
    rgr, rgroup = granges_of(rann, rnames)
    for mode in gx.MODES:
        got = bamGeneCounts(rpath, rgr, rgroup, strand=mode, paired_end="filter", mapqual=10, verbose=False)
        exp = gx.expected(rcols, rann.features, rann.gene, rann.n_genes, strand=mode, requiredF=66, mapqual=10)
        # (a model made from ranges knows the genes that have one: the others' expected counts are 0 anyway)
        known = np.asarray([rann.index(g) for g in got.genes])
        assert exp[0].sum() == exp[0][known].sum() and same((got.counts, got.summary), (exp[0][known], exp[1])), mode
    _lib.load().bsig_cache_clear()
