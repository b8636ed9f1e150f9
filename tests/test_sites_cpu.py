"""CPU: the restatement of bamSites against itself (numpy against a per-cell loop that shares no code with it), the sites deck's
planted cells read off by name, the Python layer's refusals and the AlleleSites container.  No GPU is needed: the library is
only asked for what it answers before it opens anything."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import nucleotides_expected as nx
import sites_expected as sx
from bamsignals_amd import AlleleSites, GRanges, _lib, bamSites
from bamsignals_amd.sites import fraction_of, ref_codes

GRID = [sx.prm(d, a, num, den, mask) for (d, a, num, den), mask in
        itertools.product(((1, 1, 0, 1), (3, 2, 1, 4), (2, 1, 1, 2), (9, 2, 1, 5), (1, 1, 1, 1)), (sx.MASK_WITH_DELETIONS, sx.MASK_BASES))]


@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("deck", ["hand", "random", "sites"])
def test_vectorised_is_brute(deck, ss):
    cells = sx.dense(deck, ss)
    total = 0
    for ref in (None, sx.ref_of(deck)):
        for p in GRID:
            want = sx.brute_sites(cells, ref, p)
            assert sx.same_sites(sx.expected_sites(cells, ref, p), want), (ref is None, p)
            total += len(want["pos"])
    assert total > 0


def test_ss_changes_only_what_is_reported():
    for deck in ("random", "sites"):
        for ref, p in itertools.product((None, sx.ref_of(deck)), (sx.prm(1, 1, 0, 1), sx.prm(3, 2, 1, 4))):
            one, two = sx.expected_sites(sx.dense(deck, False), ref, p), sx.expected_sites(sx.dense(deck, True), ref, p)
            assert all(np.array_equal(one[k], two[k]) for k in ("seg_off", "pos", "alleles"))
            assert np.array_equal(one["counts"], two["counts"].sum(axis=1)) and two["counts"].shape[1:] == (2, 6)


def test_both_extremes_are_exercised():
    """many sites in a range and ranges without any, on the decks of the nucleotide suite: no new data is needed for either"""
    for deck in ("hand", "random"):
        n_cells = int(np.sum(sx.deck(deck)[1]["len"]))
        for p, crowded in ((sx.prm(1, 1, 0, 1), True), (sx.prm(3, 2, 1, 4), False)):
            got = sx.expected_sites(sx.dense(deck, False), None, p)
            per = np.diff(got["seg_off"])
            assert 0 < got["seg_off"][-1] < n_cells and np.any(per == 0)
            assert per.max() >= 400 if crowded else per.max() >= 60


def planted_site(want, rg, i, x):
    """the site at genomic base x of range i: (base, alt, counts) or None"""
    cell = sx.cell_of(rg, i, x)
    a, b = int(want["seg_off"][i]), int(want["seg_off"][i + 1])
    hit = np.flatnonzero(want["pos"][a:b] == cell)
    if not len(hit):
        return None
    k = a + int(hit[0])
    return int(want["alleles"][k]) & 0xFF, int(want["alleles"][k]) >> 8, want["counts"][k]


def test_planted_sites_by_name():
    rec, rg, genome, planted = sx.sites_deck()
    ref = sx.deck_ref(rg, genome)
    want = sx.expected_sites(sx.dense("sites", False), ref, sx.NAMED)
    whole_plus, whole_minus = 5, 4          # (0, 0, 1025, *) and (0, 0, 1024, -) hold the first kilobase
    big_plus, big_minus = 6, 7
    comp = lambda ch: 3 - ch if ch < 4 else ch          # noqa: E731
    for name, i in (("het", 5), ("hom", 5), ("deletion", 5), ("alt_tie", 5), ("exact_fraction", 5), ("one_short", 5), ("ref_n", 5),
                    ("at_min_depth", 5), ("below_min_depth", 5), ("het", 4), ("deletion", 4), ("alt_tie", 4), ("at_min_depth", 4),
                    ("plus_cell_0", big_plus), ("plus_cell_1023", big_plus), ("plus_cell_1024", big_plus), ("plus_last", big_plus),
                    ("plus_last", big_minus), ("minus_cell_1023", big_minus), ("minus_cell_1024", big_minus), ("plus_cell_0", big_minus)):
        pl = planted[name]
        got = planted_site(want, rg, i, pl["x"])
        if not pl["site"]:
            assert got is None, name
            continue
        assert got is not None, name
        minus = rg["strand"][i] < 0
        b, a, counts = got
        assert (b, a) == ((comp(pl["base"]), min(comp(ch) for ch in pl["alts"])) if minus else (pl["base"], pl["alt"])), name
        assert int(counts[a]) == pl["alt_count"] and int(counts.sum()) == pl["depth"], name
    # the cells the big ranges are named for
    for name, i, cell in (("plus_cell_0", big_plus, 0), ("plus_cell_1023", big_plus, 1023), ("plus_cell_1024", big_plus, 1024),
                          ("plus_last", big_plus, 3 * nx.TILE), ("plus_last", big_minus, 0), ("minus_cell_1023", big_minus, 1023),
                          ("minus_cell_1024", big_minus, 1024), ("plus_cell_0", big_minus, 3 * nx.TILE)):
        assert sx.cell_of(rg, i, planted[name]["x"]) == cell
    # the depths and the fraction are what their names say
    assert planted["at_min_depth"]["depth"] == sx.NAMED["min_depth"] and planted["below_min_depth"]["depth"] == sx.NAMED["min_depth"] - 1
    assert planted["exact_fraction"]["alt_count"] * sx.NAMED["den"] == sx.NAMED["num"] * planted["exact_fraction"]["depth"]
    assert (planted["one_short"]["alt_count"] + 1) * sx.NAMED["den"] == sx.NAMED["num"] * planted["one_short"]["depth"]
    # two alts of 8 reads: the first channel wins, and the other one if the mask leaves the first out
    tie = planted["alt_tie"]
    first, second = sorted(((tie["base"] + 1) % 4, (tie["base"] + 2) % 4))
    assert planted_site(want, rg, whole_plus, tie["x"])[1] == first
    without = sx.expected_sites(sx.dense("sites", False), ref, dict(sx.NAMED, alt_mask=sx.MASK_BASES & ~(1 << first)))
    assert planted_site(without, rg, whole_plus, tie["x"])[1] == second
    # without deletions the deletion site is none
    bases_only = sx.expected_sites(sx.dense("sites", False), ref, dict(sx.NAMED, alt_mask=sx.MASK_BASES))
    assert planted_site(bases_only, rg, whole_plus, planted["deletion"]["x"]) is None
    # without a reference: 15 : 15 -- the first channel is the base, the other the alt; the reference N's mismatch is a site
    major = sx.expected_sites(sx.dense("sites", False), None, sx.NAMED)
    mt = planted["major_tie"]
    lo, hi = sorted((mt["base"], (mt["base"] + 1) % 4))
    assert planted_site(major, rg, whole_plus, mt["x"])[:2] == (lo, hi)
    assert planted_site(major, rg, whole_plus, planted["ref_n"]["x"]) is not None
    # a range without sites between two with sites; width 1 and 0; the reference without reads
    per = np.diff(want["seg_off"]).tolist()
    assert per[10] > 0 and per[11] == 0 and per[12] > 0
    assert per[0] == 1 and per[1] == 1 and per[2] == 0 and per[9] == 0 and per[13] == 0 and per[14] == 0
    assert per[6] == per[8] and per[6] >= 4 and per[7] >= 4, "the duplicate gives its sites twice"


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_fraction_and_ref_codes():
    assert fraction_of(0.2) == (1, 5) and fraction_of(0) == (0, 1) and fraction_of(1) == (1, 1) and fraction_of(Fraction(3, 7)) == (3, 7)
    assert fraction_of(np.float64(0.25)) == (1, 4) and fraction_of(1e-9) == (0, 1)
    num, den = fraction_of(1 / 3)
    assert den <= 1 << 20 and abs(num / den - 1 / 3) < 1e-9
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "0.2", None, True):
        with pytest.raises(ValueError, match="minFraction"):
            fraction_of(bad)
    codes = ref_codes(["ACGTN", b"acgtx-", ""], [5, 6, 0])
    assert codes.dtype == np.uint8 and codes.tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 4]
    for bad, w in ((["ACG"], [4]), (["ACG", "A"], [3]), ("ACG", [3]), ([5], [1]), (["ACé"], [3])):
        with pytest.raises(ValueError, match="ref"):
            ref_codes(bad, w)


def test_parameter_refusals(monkeypatch):
    """every parameter is refused in Python: the native library is never loaded"""
    gr = GRanges(["c1", "c1"], [1, 50], width=[4, 2], strand=["+", "-"])
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a refused call reached the library"))
    path = "/nonexistent/no.bam"
    for kw, word in ((dict(minDepth=0), "minDepth"), (dict(minDepth=2.0), "minDepth"), (dict(minDepth=True), "minDepth"), (dict(minDepth=2**31), "minDepth"),
                     (dict(minAlt=0), "minAlt"), (dict(minAlt="2"), "minAlt"), (dict(minFraction=-0.5), "minFraction"), (dict(minFraction=1.01), "minFraction"),
                     (dict(minFraction="x"), "minFraction"), (dict(deletions=1), "deletions"), (dict(mapqual=256), "mapqual"),
                     (dict(filteredFlag=-2), "filteredFlag"), (dict(minBaseQuality=94), "minBaseQuality"), (dict(ss=1), "ss"),
                     (dict(ref=["ACGT"]), "ref"), (dict(ref=["ACG", "AC"]), "ref"), (dict(ref="ACGTAC"), "ref")):
        with pytest.raises(ValueError, match=word):
            bamSites(path, gr, verbose=False, **kw)
    with pytest.raises(TypeError, match="GRanges"):
        bamSites(path, [("c1", 1, 10)], verbose=False)


SITES_ARGS = dict(mapqual=0, requiredF=0, filteredF=-1, min_base_qual=0, ss=0, ref=None, min_depth=1, min_alt=1, frac_num=0, frac_den=1, alt_mask=0x2F)


def native_sites(**kw):
    """bsig_sites on a path that does not exist, without ranges: what the library says before it opens anything"""
    a = dict(SITES_ARGS, **kw)
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.bsig_sites(b"/nonexistent/no.bam", a.get("n", 0), None, 0, None, None, a.get("width"), None, a["mapqual"], a["requiredF"], a["filteredF"],
                        a["min_base_qual"], a["ss"], a["ref"], a["min_depth"], a["min_alt"], a["frac_num"], a["frac_den"], a["alt_mask"], -1, C.byref(h))
    assert not h.value
    return _lib.ERR_NAMES[rc], lib.bsig_last_error().decode()


def test_the_library_judges_its_parameters_before_it_opens_the_file():
    sentences = set()
    for kw, word in ((dict(min_depth=0), "min_depth must be at least 1"), (dict(min_alt=0), "min_alt must be at least 1"),
                     (dict(frac_den=0), "frac_den must lie between 1 and 2^20"), (dict(frac_den=(1 << 20) + 1), "frac_den must lie between 1 and 2^20"),
                     (dict(frac_num=-1), "frac_num must lie between 0 and frac_den"), (dict(frac_num=3, frac_den=2), "frac_num must lie between 0 and frac_den"),
                     (dict(alt_mask=0), "alt_mask"), (dict(alt_mask=0x40), "alt_mask"), (dict(min_base_qual=94), "min_base_qual must lie between 0 and 93")):
        code, msg = native_sites(**kw)
        assert code == "BSIG_ERR_ARG" and word in msg, (kw, msg)
        sentences.add(word)
    assert len(sentences) == 6, "each refusal has a sentence of its own"
    # a reference code above 4, judged from the widths alone
    width = np.asarray([3, 0, 2], dtype=np.int32)
    ref = np.asarray([0, 4, 1, 2, 5], dtype=np.uint8)
    code, msg = native_sites(n=3, width=width.ctypes.data, ref=ref.ctypes.data)
    assert code == "BSIG_ERR_ARG" and "code 5 at cell 1 of range 2" in msg
    # ... and parameters that pass reach the file, which is not there
    assert native_sites()[0] == "BSIG_ERR_IO"
    assert native_sites(frac_num=1 << 20, frac_den=1 << 20, min_depth=2**31 - 1, min_alt=2**31 - 1, alt_mask=1)[0] == "BSIG_ERR_IO"


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("bsig_reads_sites", "bsig_sites", "bsig_sites_result_n_ranges", "bsig_sites_result_n_sites", "bsig_sites_result_copy",
                 "bsig_sites_result_timing", "bsig_sites_result_free"):
        assert hasattr(lib, name), name
    assert lib.bsig_sites_result_n_ranges(None) == 0 and lib.bsig_sites_result_n_sites(None) == 0
    lib.bsig_sites_result_free(None)


# ---- the container -----------------------------------------------------------------------------------------------------------------
def test_allele_sites_from_hand_made_integers():
    counts = np.asarray([[10, 5, 0, 0, 0, 0], [0, 0, 2, 0, 0, 6], [1, 1, 1, 9, 0, 0]], dtype=np.int32)
    s = AlleleSites([0, 2, 2, 3], [1, 3, 0], [0, 5, 3], [1, 2, 0], counts)
    assert len(s) == 3 and s.nsites == 3 and not s.ss and s.channels == ("A", "C", "G", "T", "N", "-")
    assert s.range_index().tolist() == [0, 0, 2] and s.depth().tolist() == [15, 8, 12] and s.alt_count().tolist() == [5, 2, 1]
    assert s.alt_fraction().tolist() == [5 / 15, 2 / 8, 1 / 12]
    assert s[0]["pos"].tolist() == [1, 3] and s[1]["pos"].tolist() == [] and s[-1]["alt"].tolist() == [0]
    gr = GRanges(["c1", "c2", "c1"], [101, 7, 201], width=[5, 0, 4], strand=["-", "+", "*"])
    assert s.genomic_pos(gr).tolist() == [104, 102, 201], "a '-' range counts down from its last base"
    t = s.to_table(gr)
    assert t["seqnames"] == ["c1", "c1", "c1"] and t["pos"].tolist() == [104, 102, 201] and t["range"].tolist() == [0, 0, 2]
    assert t["A"].tolist() == [10, 0, 1] and t["-"].tolist() == [0, 6, 0] and t["ref"] == ["A", "-", "T"] and t["alt"] == ["C", "G", "A"]
    assert set(t) == {"seqnames", "pos", "range", "A", "C", "G", "T", "N", "-", "ref", "alt"}
    # read-only
    for a in (s.seg_off, s.pos, s.base, s.alt, s.counts):
        assert not a.flags.writeable
        with pytest.raises(ValueError):
            a[...] = 0
    # with ss: the planes are summed for every figure
    both = AlleleSites([0, 3], [1, 3, 4], [0, 5, 3], [1, 2, 0], np.stack([counts, 2 * counts], axis=1), ss=True)
    assert both.counts.shape == (3, 2, 6) and both.depth().tolist() == [45, 24, 36] and both.alt_count().tolist() == [15, 6, 3]
    # an empty result
    none = AlleleSites([0, 0, 0], [], [], [], np.zeros((0, 6), dtype=np.int32))
    assert len(none) == 2 and none.nsites == 0 and none.depth().tolist() == [] and none.alt_fraction().tolist() == []
    gr2 = GRanges(["c1", "c1"], [1, 9], width=[3, 3], strand=["+", "-"])
    assert none.genomic_pos(gr2).tolist() == [] and none.to_table(gr2)["pos"].tolist() == [] and none.to_table(gr2)["ref"] == []
    assert AlleleSites([0], [], [], [], np.zeros((0, 2, 6), dtype=np.int32), ss=True).nsites == 0
    for bad in (dict(seg_off=[0, 2, 2, 4]), dict(seg_off=[1, 2, 2, 3]), dict(alt=[0, 2, 0]), dict(base=[0, 6, 3]), dict(pos=[1, -3, 0])):
        args = dict(seg_off=[0, 2, 2, 3], pos=[1, 3, 0], base=[0, 5, 3], alt=[1, 2, 0], counts=counts)
        args.update(bad)
        with pytest.raises(ValueError):
            AlleleSites(**args)
    with pytest.raises(ValueError):
        s.genomic_pos(gr[0])
    with pytest.raises(ValueError):
        s.genomic_pos(GRanges(["c1", "c2", "c1"], [101, 7, 201], width=[3, 0, 4], strand=["-", "+", "*"]))       # a site beyond its range
    with pytest.raises(IndexError):
        s[3]
    with pytest.raises(TypeError):
        s["0"]


def test_to_bed(tmp_path):
    counts = np.asarray([[10, 5, 0, 0, 0, 0], [1, 1, 1, 9, 0, 0]], dtype=np.int32)
    s = AlleleSites([0, 1, 2], [1, 0], [0, 3], [1, 0], counts)
    gr = GRanges(["c1", "c2"], [101, 201], width=[5, 4], strand=["-", "*"])
    path = tmp_path / "sites.bed"
    assert s.to_bed(str(path), gr) == 2
    assert path.read_text() == "c1\t103\t104\tA>C\t333\t-\nc2\t200\t201\tT>A\t83\t.\n"
