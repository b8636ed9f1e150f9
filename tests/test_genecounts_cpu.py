"""CPU: the gene counts' expected side (tests/genecounts_expected.py: every block against every feature, never flattened)
against a brute force with Python sets; the host-side gene model (bsig_gene_model_*: csrc/genemodel.h through the C ABI)
against a per-base restatement; the proof that deciding a read from the flattened tables equals the set rule; the decks'
properties; GeneModel, GeneCounts and bamGeneCounts' own refusals -- none of which needs a device."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import genecounts_expected as gx
import junctions_expected as jx

BAM = os.path.join(GOLDEN, "randomBam.bam")
I32 = np.int32
FILTERS = (dict(), dict(mapqual=30, filteredF=0x400), dict(requiredF=66))


def test_the_package_exports_the_feature():
    import bamsignals_amd
    assert callable(bamsignals_amd.bamGeneCounts) and isinstance(bamsignals_amd.GeneCounts, type) and isinstance(bamsignals_amd.GeneModel, type)
    assert {"bamGeneCounts", "GeneCounts", "GeneModel"} <= set(bamsignals_amd.__all__)
    for words in ("intersection-strict", "minOverlap", "fracOverlap", "-O", "ONE fragment"):
        assert words in bamsignals_amd.genecounts.__doc__, "what is not built is said"


def model_of(ann, n_ref):
    from bamsignals_amd import GeneModel
    f = ann.features
    return GeneModel.from_arrays(f["rid"], f["loc"], f["len"], f["strand"], ann.gene, ann.n_genes, n_ref, genes=ann.labels)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", gx.MODES)
@pytest.mark.parametrize("deck", ["hand", "junction", "junction_stretched"])
def test_restatement_is_the_brute_force(deck, mode):
    cols, ann = gx.deck(deck)
    for flt in FILTERS:
        want = gx.brute_outcomes(cols, ann.features, ann.gene, ann.n_genes, strand=mode, **flt)
        got = gx.outcomes(cols, ann.features, ann.gene, ann.n_genes, strand=mode, **flt)
        assert np.array_equal(got, want), flt
        counts, summary = gx.tally(got, ann.n_genes)
        assert summary.sum() == len(cols["pos"]) and counts.sum() == summary[0] and len(counts) == ann.n_genes


def test_hand_cases():
    cols, ann, at = gx.hand()
    out = {m: gx.outcomes(cols, ann.features, ann.gene, ann.n_genes, strand=m) for m in gx.MODES}
    un, fw, rv = (out[m] for m in gx.MODES)
    g = ann.index
    # a feature ending one base before a block starts, and one ending on its first base; the same at the block's end
    assert un[at["before_start"]] == gx.NO_FEATURE and un[at["on_start"]] == g("E1")
    assert un[at["behind_end"]] == gx.NO_FEATURE and un[at["on_end"]] == g("E3")
    # one gene through two exons counts once; two genes through two blocks are ambiguous; a read inside an overlap is ambiguous
    assert un[at["two_exons"]] == g("X2") and fw[at["two_exons"]] == g("X2") and rv[at["two_exons"]] == gx.NO_FEATURE
    assert un[at["two_genes"]] == gx.AMBIGUOUS and un[at["inside_ambig"]] == gx.AMBIGUOUS
    # a gene nested in another's intron: the read spliced over it belongs to the outer gene, the unspliced one inside it to
    # the inner gene.  bamOverlaps takes a read as the one interval [first base, last base]: it would put the spliced read
    # on INNER as well (its span 14,050 .. 15,049 holds 14,400 .. 14,600) and so call it ambiguous
    assert un[at["over_nested"]] == g("OUTER") and un[at["in_nested"]] == g("INNER")
    k = at["over_nested"]
    f = ann.features
    inner = np.flatnonzero(ann.gene == g("INNER"))[0]
    assert cols["pos"][k] <= f["loc"][inner] and cols["end"][k] >= f["loc"][inner] + f["len"][inner] - 1
    # exons that touch with no base between
    assert un[at["touch_left"]] == g("F1") and un[at["touch_right"]] == g("F2") and un[at["touch_both"]] == gx.AMBIGUOUS
    assert fw[at["touch_both"]] == g("F1") and rv[at["touch_both"]] == g("F2")
    # two transcripts of one gene
    assert un[at["transcripts"]] == g("T")
    # antisense genes: ambiguous, resolved, swapped
    assert un[at["anti_fwd"]] == un[at["anti_rev"]] == gx.AMBIGUOUS
    assert (fw[at["anti_fwd"]], fw[at["anti_rev"]]) == (g("P"), g("M")) and (rv[at["anti_fwd"]], rv[at["anti_rev"]]) == (g("M"), g("P"))
    # a '*' feature matches under every mode
    assert all(o[at[k]] == g("S") for o in (un, fw, rv) for k in ("star_fwd", "star_rev"))
    # second mates lie on the other strand of their fragment
    assert (fw[at["mate2_rev"]], fw[at["mate2_fwd"]], fw[at["mate1_rev"]]) == (g("J"), gx.NO_FEATURE, gx.NO_FEATURE)
    assert (rv[at["mate2_rev"]], rv[at["mate2_fwd"]], rv[at["mate1_rev"]]) == (gx.NO_FEATURE, g("J"), g("J"))
    # an intron over 1,100 genes; the read of 35,000 blocks meets a feature with its last block alone
    assert un[at["long_intron"]] == g("KA") and un[at["stepping_398"]] == g("K398")
    assert un[at["long_read"]] == g("L")
    counts, summary = gx.tally(un, ann.n_genes)
    assert counts[g("L_GAP")] == 0 and counts[g("Z")] == 0 and counts[g("NO_FEATURE_GENE")] == 0 and counts[g("N1")] == 0
    assert un[at["no_features_here"]] == gx.NO_FEATURE and summary[4] == 1
    m = model_of(ann, len(cols["ref_len"]))
    seg = m.segments("unstranded")
    a, b = np.searchsorted(seg["start"][:seg["ref_off"][1]], [30_050, 90_049])
    assert b - a > 1_000, "the long intron skips more than 1,000 segments"
    assert seg["ref_off"][1] == seg["ref_off"][2] and seg["ref_off"][4] == seg["ref_off"][5] and seg["ref_off"][3] < seg["ref_off"][4]
    assert cols["ref_off"][1] == cols["ref_off"][2] and cols["ref_off"][3] == cols["ref_off"][4] < cols["ref_off"][5]


def test_junction_deck_annotation():
    cols, ann = gx.junction()
    want = jx.junction_genes()
    f = ann.features
    for k in range(20):
        mine = np.flatnonzero(ann.gene == k)
        assert f["rid"][mine[0]] == want["rid"][k] and f["loc"][mine].min() == want["loc"][k] and set(f["strand"][mine]) == {want["strand"][k]}
        assert (f["loc"][mine] + f["len"][mine]).max() == want["loc"][k] + want["len"][k], "the replay is the deck's own exons"
    counts, summary = gx.expected(cols, f, ann.gene, ann.n_genes)
    assert counts.tolist() == list(jx.READS_PER_GENE) * 2 and summary.tolist() == [2 * sum(jx.READS_PER_GENE), 0, 0, 0, 0]
    fwd = gx.expected(cols, f, ann.gene, ann.n_genes, strand="forward")[1]
    assert 0.05 < fwd[2] / summary[0] < 0.15, "10 % of the strands are flipped"
    _, stretched = gx.junction(True)
    out = gx.outcomes(cols, stretched.features, stretched.gene, stretched.n_genes)
    c2, s2 = gx.tally(out, stretched.n_genes)
    assert s2[1] > 100 and s2[0] + s2[1] == summary[0]
    # every gene with a neighbour before it opens with a run of ambiguous reads: 18 such genes, two breaks each or nearly
    assert np.count_nonzero(np.diff(out) != 0) >= 30


@pytest.mark.parametrize("mode", gx.MODES)
def test_random_deck_has_every_category(mode):
    cols, ann = gx.random()
    assert len(cols["pos"]) == 5000 and ann.n_genes == gx.RANDOM_GENES
    counts, summary = gx.expected(cols, ann.features, ann.gene, ann.n_genes, strand=mode, mapqual=30, filteredF=0x400)
    assert np.all(summary > 0), summary
    assert np.count_nonzero(counts) >= 20
    counts, summary = gx.expected(cols, ann.features, ann.gene, ann.n_genes, strand=mode)
    assert np.all(summary[[0, 1, 2, 4]] > 0) and summary[3] == 0 and np.count_nonzero(counts) >= 20
    counts, summary = gx.expected(cols, ann.features, ann.gene, ann.n_genes, strand=mode, requiredF=66)
    assert np.all(summary > 0) and np.count_nonzero(counts) >= 20


# ---- the gene model through the ABI -------------------------------------------------------------------------------------------
def small_annotations():
    rng = np.random.default_rng(77)
    out = []
    for n_feat, n_genes in ((0, 3), (1, 1), (40, 6), (200, 25), (200, 2)):
        feats = []
        for _ in range(n_feat):
            rid = int(rng.integers(0, 3))
            a = int(rng.integers(0, 2_900))
            w = int(rng.integers(0, 100))
            feats.append((int(rng.integers(0, n_genes)), rid, a, a + w - 1, int(rng.integers(-1, 2))))
        out.append((gx.Annotation(feats, labels=list(range(n_genes))), [3_000, 3_000, 3_000]))
    hand = [(0, 0, 10, 19, 1), (0, 0, 20, 29, 1), (1, 0, 30, 39, 1), (1, 0, 35, 50, -1), (0, 0, 45, 60, 0), (2, 0, 0, 0, 1),
            (2, 0, 2_999, 2_999, -1), (3, 0, 100, 99, 1), (0, 2, 5, 9, 1), (1, 2, 10, 14, 1), (0, 2, 15, 19, 1)]
    out.append((gx.Annotation(hand, labels=[0, 1, 2, 3, 4]), [3_000, 10, 3_000]))
    return out


@pytest.mark.parametrize("table", gx.TABLES)
def test_model_is_the_per_base_flatten(table):
    for ann, ref_len in small_annotations():
        m = model_of(ann, len(ref_len))
        got, want = m.segments(table), gx.flatten_brute(ann.features, ann.gene, table, ref_len)
        assert m.n_segments(table) == len(want["start"])
        for k in ("ref_off", "start", "end", "value"):
            assert np.array_equal(got[k], want[k]), (table, k)
        assert got["ref_off"].dtype == np.int64 and got["value"].dtype == I32
        m.close()


def test_touching_segments_merge_and_overlaps_are_ambiguous():
    ann, ref_len = small_annotations()[-1]
    seg = model_of(ann, 3).segments("unstranded")
    r0 = slice(0, seg["ref_off"][1])
    assert list(zip(seg["start"][r0], seg["end"][r0], seg["value"][r0])) == \
        [(0, 0, 2), (10, 29, 0), (30, 44, 1), (45, 50, -1), (51, 60, 0), (2_999, 2_999, 2)]
    r2 = slice(seg["ref_off"][2], seg["ref_off"][3])
    assert list(zip(seg["start"][r2], seg["end"][r2], seg["value"][r2])) == [(5, 9, 0), (10, 14, 1), (15, 19, 0)]
    plus = model_of(ann, 3).segments("plus")
    assert list(zip(plus["start"], plus["end"], plus["value"]))[1:4] == [(10, 29, 0), (30, 39, 1), (45, 60, 0)]


@pytest.mark.parametrize("mode", gx.MODES)
@pytest.mark.parametrize("deck", gx.DECKS)
def test_deciding_from_the_tables_is_the_set_rule(deck, mode):
    """the trick the kernel relies on, proven without it: walk the segments a read's blocks touch in one flattened table"""
    cols, ann = gx.deck(deck)
    m = model_of(ann, len(cols["ref_len"]))
    tables = {t: m.segments(t) for t in gx.TABLES}
    for flt in FILTERS[:2]:
        want = gx.outcomes(cols, ann.features, ann.gene, ann.n_genes, strand=mode, **flt)
        assert np.array_equal(gx.decide_from_segments(cols, tables, strand=mode, **flt), want), flt
    again = model_of(ann.twice_and_reversed(), len(cols["ref_len"]))
    for t in gx.TABLES:
        assert all(np.array_equal(again.segments(t)[k], tables[t][k]) for k in tables[t]), "features given twice and reversed"


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _create(rid=(0,), loc=(0,), ln=(10,), strand=(0,), gene=(0,), n_genes=1, n_ref=1):
    from bamsignals_amd import _lib
    lib = _lib.load()
    a = [np.asarray(x, I32) for x in (rid, loc, ln, strand, gene)]
    h = C.c_void_p()
    rc = lib.bsig_gene_model_create(len(a[0]), *[x.ctypes.data for x in a], n_genes, n_ref, C.byref(h))
    if h.value:
        lib.bsig_gene_model_free(h)
    return rc, lib.bsig_last_error().decode()


@pytest.mark.parametrize("a, words", [
    (dict(rid=(0, 0), loc=(0, 5), ln=(10, -1), strand=(0, 0), gene=(0, 0)), "feature 1 has a negative width"),
    (dict(rid=(1,)), "feature 0: reference 1 is not one of the model's 1"),
    (dict(rid=(-1,)), "feature 0: reference -1 is not one of the model's 1"),
    (dict(gene=(1,)), "feature 0: gene 1 is not one of the model's 1"),
    (dict(gene=(-1,)), "feature 0: gene -1 is not one of the model's 1"),
    (dict(rid=(0, 0, 0), loc=(0, 0, 0), ln=(1, 1, 1), strand=(0, 1, 2), gene=(0, 0, 0)), "feature 2: strand 2 is none of -1, 0, 1"),
    (dict(strand=(-2,)), "feature 0: strand -2 is none of -1, 0, 1"),
    (dict(loc=(2**31 - 10,), ln=(10,)), "feature 0 ends beyond base 2^31 - 1"),
])
def test_model_refusals(a, words):
    rc, msg = _create(**a)
    assert rc == -1 and msg == words


def test_model_accepts_the_edges():
    assert _create(loc=(2**31 - 11,), ln=(10,))[0] == 0
    assert _create(rid=(), loc=(), ln=(), strand=(), gene=(), n_genes=4, n_ref=2)[0] == 0
    from bamsignals_amd import _lib
    lib = _lib.load()
    assert lib.bsig_gene_model_n_segments(None, 0) == -1 and lib.bsig_reads_n_source_reads(None) == 0


def test_gene_model_class():
    from bamsignals_amd import GeneModel, GRanges
    gr = GRanges(["c2", "c1", "c2", "c1"], [11, 1, 31, 5], width=[10, 100, 10, 0], strand=["+", "-", "+", "*"])
    m = GeneModel(gr, ["b", "a", "b", "z"])
    assert m.genes == ("b", "a", "z") and m.seqlevels == ("c2", "c1") and len(m) == 3 and (m.n_features, m.n_ref) == (4, 2)
    seg = m.segments()
    assert seg["ref_off"].tolist() == [0, 2, 3] and seg["start"].tolist() == [10, 30, 0] and seg["end"].tolist() == [19, 39, 99]
    assert seg["value"].tolist() == [0, 0, 1] and m.n_segments("minus") == 1 and m.n_segments(1) == 2
    assert "3 genes, 4 features, 3 segments" in repr(m)
    assert GeneModel(gr, np.asarray([7, 3, 7, 5])).genes == (7, 3, 5)
    for bad, words in (((gr, ["a", "b"]), "one label per range"), ((gr, "abcd"), "one label per range"), ((gr, None), "one label per range")):
        with pytest.raises(ValueError, match=words):
            GeneModel(*bad)
    with pytest.raises(TypeError, match="GRanges"):
        GeneModel([("c1", 1, 10)], ["a"])
    with pytest.raises(ValueError, match="table must be one of"):
        m.segments("both")
    with pytest.raises(ValueError, match="whole numbers"):
        GeneModel.from_arrays([0.5], [0], [1], [0], [0], 1, 1)
    from bamsignals_amd import _lib
    with pytest.raises(_lib.BsigError, match="feature 0: gene 3 is not one of the model's 2"):
        GeneModel.from_arrays([0], [0], [1], [0], [3], 2, 1)


def _counts(many):
    from bamsignals_amd import GeneCounts
    if many:
        return GeneCounts(["a", "b", "c"], [[5, 1], [0, 0], [7, 2]], [[12, 3, 4, 1, 0], [3, 0, 0, 0, 0]], files=["x.bam", "y.bam"])
    return GeneCounts(["a", "b", "c"], [5, 0, 7], [12, 3, 4, 1, 0])


def test_gene_counts_class(tmp_path):
    from bamsignals_amd import GeneCounts
    one, two = _counts(False), _counts(True)
    assert len(one) == 3 and one.counts.dtype == np.int64 and one.counts.shape == (3,) and two.counts.shape == (3, 2)
    assert (one.assigned, one.ambiguous, one.no_feature, one.filtered, one.unmapped) == (12, 3, 4, 1, 0) and one.n_reads == 20
    assert two.assigned.tolist() == [12, 3] and two.unmapped.tolist() == [0, 0] and two.n_reads.tolist() == [20, 3]
    assert one.assigned_fraction() == 0.6 and two.assigned_fraction().tolist() == [0.6, 1.0]
    assert GeneCounts([], [], [0, 0, 0, 0, 0]).assigned_fraction() == 0.0
    assert "3 genes, 1 file, 12 of 20 reads assigned" in repr(one) and "3 genes, 2 files, 15 of 23 reads assigned" in repr(two)
    for a in (one.counts, one.summary, two.counts, two.summary):
        with pytest.raises(ValueError):
            a[...] = 0
    with pytest.raises(AttributeError):
        one.nothing
    p = str(tmp_path / "c.tsv")
    assert one.to_tsv(p) == 8
    assert open(p).read() == "a\t5\nb\t0\nc\t7\n__assigned\t12\n__ambiguous\t3\n__no_feature\t4\n__filtered\t1\n__unmapped\t0\n"
    assert two.to_tsv(p) == 8
    assert open(p).read() == ("a\t5\t1\nb\t0\t0\nc\t7\t2\n__assigned\t12\t3\n__ambiguous\t3\t0\n__no_feature\t4\t0\n"
                              "__filtered\t1\t0\n__unmapped\t0\t0\n")
    for bad in (dict(counts=[5, 0]), dict(counts=[5, 0, 6]), dict(counts=[5, -1, 8]), dict(summary=[12, 3, 4, 1]), dict(files=["a", "b"])):
        a = dict(genes=["a", "b", "c"], counts=[5, 0, 7], summary=[12, 3, 4, 1, 0])
        a.update(bad)
        with pytest.raises(ValueError):
            GeneCounts(**a)


def test_bamgenecounts_refuses_bad_arguments_before_any_file_is_opened(monkeypatch):
    from bamsignals_amd import GeneModel, GRanges, _lib, bamGeneCounts
    gr = GRanges(["chr1"], [1], width=[100])
    model = GeneModel(gr, ["a"])

    def no_call(*a, **k):
        raise AssertionError("the file-level call was made")
    monkeypatch.setattr(_lib.load(), "bsig_gene_counts", no_call, raising=False)
    for kw, words in ((dict(mapqual=-1), "mapqual"), (dict(mapqual=256), "mapqual"), (dict(mapqual=1.5), "mapqual"),
                      (dict(mapqual=True), "mapqual"), (dict(filteredFlag="x"), "filteredFlag"), (dict(filteredFlag=1 << 16), "filteredFlag"),
                      (dict(strand="sense"), "strand must be one of"), (dict(strand=1), "strand must be one of"),
                      (dict(paired_end="extend"), "paired.end"), (dict(verbose=1), "verbose must be True or False")):
        with pytest.raises(ValueError, match=words):
            bamGeneCounts(BAM, gr, ["a"], **{"verbose": False, **kw})
    with pytest.raises(TypeError, match="GRanges"):
        bamGeneCounts(BAM, [("chr1", 1, 100)], ["a"], verbose=False)
    with pytest.raises(ValueError, match="one label per range"):
        bamGeneCounts(BAM, gr, None, verbose=False)
    with pytest.raises(ValueError, match="group must be None"):
        bamGeneCounts(BAM, model, ["a"], verbose=False)
    with pytest.raises(ValueError, match="holds no path"):
        bamGeneCounts([], model, verbose=False)
    with pytest.raises(ValueError, match="without sequence names"):
        bamGeneCounts(BAM, GeneModel.from_arrays([0], [0], [1], [0], [0], 1, 1), verbose=False)


def _call(strandedness=0, model=True, counts=True, summary=True, path=BAM, levels=(b"chr1", b"chr2"), n_ref=2):
    from bamsignals_amd import _lib
    lib = _lib.load()
    a = [np.asarray(x, I32) for x in ((0, 1), (1000, 1000), (100, 100), (1, -1), (0, 1))]
    h = C.c_void_p()
    assert lib.bsig_gene_model_create(2, *[x.ctypes.data for x in a], 2, n_ref, C.byref(h)) == 0
    names = (C.c_char_p * len(levels))(*levels)
    c, s = np.full(2, -7, np.int64), np.full(5, -7, np.int64)
    rc = lib.bsig_gene_counts(path.encode(), h if model else None, len(levels), names, 0, 0, -1, strandedness, -1,
                              c.ctypes.data if counts else None, s.ctypes.data if summary else None)
    lib.bsig_gene_model_free(h)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


MISSING = os.path.join(GOLDEN, "no_such_file.bam")


@pytest.mark.parametrize("a, want", [
    (dict(strandedness=3), (-1, "strandedness must be 0 (unstranded), 1 (forward) or 2 (reverse): 3 given")),
    (dict(strandedness=-1, path=MISSING), (-1, "strandedness must be 0 (unstranded), 1 (forward) or 2 (reverse): -1 given")),
    (dict(model=False), (-1, "model is NULL")),
    (dict(summary=False, path=MISSING), (-1, "counts or summary is NULL")),
    (dict(counts=False), (-1, "counts or summary is NULL")),
    (dict(levels=(b"chr1",)), (-1, "the gene model has 2 references, 1 sequence names were given")),
    (dict(path=MISSING), (-2, "Fail to open BAM file <missing>")),
    (dict(levels=(b"chr1", b"chrNone")), (-4, "chromosome chrNone not present in the bam file")),
])
def test_parameter_rule_at_file_level(a, want):
    rc, msg, route = _call(**a)
    assert (rc, msg.replace(MISSING, "<missing>")) == want
    assert route == b""                                  # refused: before the BAM is opened where the parameters are at fault


def test_file_level_refuses_without_a_gpu():
    """as every other compute call: no device, no quiet fall-back"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    rc, msg, _ = _call()
    assert rc != 0 and msg
    from bamsignals_amd import GRanges, _lib, bamGeneCounts
    with pytest.raises(_lib.BsigError):
        bamGeneCounts(BAM, GRanges(["chr1"], [1000], width=[100]), ["a"], verbose=False)
