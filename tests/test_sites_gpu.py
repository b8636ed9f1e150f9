"""GPU: the variant and mixed-allele sites at handle level (Reads.sites) and at file level (bamSites), against
tests/sites_expected.py: the restatement of the decision over tests/nucleotides_expected.py's restatement of the counts.
Expectations of files come from that module's own BAM reader, never from the library's decode.  All results are integers and
compared exactly."""
import itertools

import numpy as np
import pytest

import nucleotides_expected as nx
import sites_expected as sx
from bamsignals_amd import BamFile, _lib, bamNucleotides, bamSites
from bamsignals_amd.device import Context, Reads
from bamsignals_amd.sites import ref_codes
from bamsignals_amd.wrappers import last_call_route, last_call_timing

pytestmark = pytest.mark.gpu

DECKS = ("hand", "random", "sites")
PARAMS = (sx.prm(1, 1, 0, 1), sx.prm(3, 2, 1, 4), sx.prm(2, 1, 1, 2))
MASKS = (sx.MASK_WITH_DELETIONS, sx.MASK_BASES)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def upload(ctx, rec, bases=True, spliced=False):
    extra = dict(bases=True, seq_off=rec["seq_off"], seq=nx.packed(rec), qual=rec["qual"]) if bases else dict(spliced=spliced)
    return Reads(ctx, rec["ref_len"], rec["ref_off"], rec["pos"], rec["flag"], rec["mapq"], rec["tlen"],
                 cigar_off=rec["cigar_off"], cigar=rec["cigar"], **extra)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, names, the records the independent reader finds in the file, ranges, reference): written once, left
    unchanged"""
    d = tmp_path_factory.mktemp("sites")
    out = {}
    for name in DECKS:
        rec, rg, names = sx.deck(name)
        path = nx.write_bam(d / f"{name}.bam", names, rec)
        out[name] = (path, names, nx.read_bam(path)[1], rg, sx.ref_of(name))
    return out


@pytest.fixture(scope="module")
def sets(ctx, files):
    """name -> the resident set with bases, uploaded from the reader's records"""
    out = {name: upload(ctx, f[2]) for name, f in files.items()}
    yield out
    for r in out.values():
        r.close()


_dense = {}


def dense(files, deck, ss, **flt):
    """the restatement of the counts on the deck's own ranges, computed once per filter"""
    key = (deck, tuple(sorted(flt.items())))
    if key not in _dense:
        _dense[key] = nx.expected(files[deck][2], files[deck][3], ss=True, **flt)
    return _dense[key] if ss else [a.sum(axis=0, dtype=np.int32) for a in _dense[key]]


def query(reads, rg, p, ref=None, **kw):
    return reads.sites(rg["rid"], rg["loc"], rg["len"], rg["strand"], ref=None if ref is None else sx.flat_ref(ref), min_depth=p["min_depth"],
                       min_alt=p["min_alt"], frac=(p["num"], p["den"]), alt_mask=p["alt_mask"], **kw)


def check_all(reads, files, deck):
    """every combination the suite names, on one set; returns (sites seen, ranges seen without any)"""
    rg, ref = files[deck][3], files[deck][4]
    n_sites = n_bare = 0
    for ss, flt, use_ref, (p, mask) in itertools.product((False, True), sx.FILTERS, (True, False), zip(PARAMS, itertools.cycle(MASKS))):
        p = dict(p, alt_mask=mask)
        got = query(reads, rg, p, ref if use_ref else None, ss=ss, **flt)
        want = sx.expected_sites(dense(files, deck, ss, **flt), ref if use_ref else None, p)
        assert sx.same_sites(got, want), (ss, flt, use_ref, p)
        assert got[0].dtype == np.int64 and all(a.dtype == np.int32 for a in got[1:]) and got[3].shape == ((len(got[1]), 2, 6) if ss else (len(got[1]), 6))
        n_sites += len(got[1])
        n_bare += int(np.sum(np.diff(got[0]) == 0))
    return n_sites, n_bare


# ---- the query == the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck", DECKS)
def test_uploaded_sets_give_the_restatement(files, sets, deck):
    n_sites, n_bare = check_all(sets[deck], files, deck)
    assert n_sites > 0 and n_bare > 0, "sites exist, and some ranges have none"


@pytest.mark.parametrize("deck", DECKS)
def test_sets_decoded_from_the_file_give_the_restatement(ctx, files, deck):
    bam = BamFile(files[deck][0])
    reads = Reads.from_bam(ctx, bam, bases=True)
    try:
        n_sites, n_bare = check_all(reads, files, deck)
    finally:
        reads.close()
        bam.close()
    assert n_sites > 0 and n_bare > 0


def test_planted_sites(files, sets):
    """the sites deck's cells under the parameters they are named for, with the deck's own reference"""
    _, rg, genome, planted = sx.sites_deck()
    ref = sx.deck_ref(rg, genome)
    for ss in (False, True):
        got = query(sets["sites"], rg, sx.NAMED, ref, ss=ss)
        assert sx.same_sites(got, sx.expected_sites(dense(files, "sites", ss), ref, sx.NAMED))
    seg, pos = got[0], got[1]
    at = lambda i, name: sx.cell_of(rg, i, planted[name]["x"]) in pos[seg[i]:seg[i + 1]].tolist()          # noqa: E731
    assert at(5, "het") and at(5, "exact_fraction") and at(5, "at_min_depth") and at(4, "deletion")
    assert not at(5, "one_short") and not at(5, "below_min_depth") and not at(5, "ref_n")
    assert all(at(6, n) for n in ("plus_cell_0", "plus_cell_1023", "plus_cell_1024", "plus_last"))
    assert all(at(7, n) for n in ("plus_last", "minus_cell_1023", "minus_cell_1024", "plus_cell_0"))


def test_a_full_tile(files, sets):
    """a reference that is the complement of what the reads show: every covered cell of a 2,049-wide '-' range is a site -- 1,024
    in one tile, and the last tile holds one cell"""
    _, _, genome, _ = sx.sites_deck()
    rg = dict(rid=np.int32([0]), loc=np.int32([1000]), len=np.int32([2 * nx.TILE + 1]), strand=np.int32([-1]))
    shown = sx.deck_ref(rg, np.where(genome == 4, 0, genome))[0]             # what a '-' range reads: reversed, complemented
    ref = [(3 - shown).astype(np.uint8)]
    for ss in (False, True):
        got = query(sets["sites"], rg, sx.prm(1, 1, 0, 1), ref, ss=ss)
        assert got[0].tolist() == [0, 2 * nx.TILE + 1] and np.array_equal(got[1], np.arange(2 * nx.TILE + 1))
        assert sx.same_sites(got, sx.expected_sites(nx.expected(files["sites"][2], rg, ss=ss), ref, sx.prm(1, 1, 0, 1)))


@pytest.mark.parametrize("deck", DECKS)
def test_ranges_reversed_and_twice(files, sets, deck):
    reads, rg, ref = sets[deck], files[deck][3], files[deck][4]
    n = len(rg["rid"])
    order = np.concatenate([np.arange(n)[::-1], np.arange(n)])
    twice = {k: v[order] for k, v in rg.items()}
    for ss, use_ref, p in ((False, True, PARAMS[0]), (True, False, PARAMS[1])):
        cells = dense(files, deck, ss)
        r2 = [ref[i] for i in order] if use_ref else None
        want = sx.expected_sites([cells[i] for i in order], r2, p)
        got = query(reads, twice, p, r2, ss=ss)
        assert sx.same_sites(got, want)
        assert sx.same_sites(query(reads, twice, p, r2, ss=ss), dict(zip(("seg_off", "pos", "alleles", "counts"), got))), "a second run gives the same arrays"
        assert len(got[1]) > 0


def test_no_site_at_all(files, sets):
    rg = files["random"][3]
    for ss in (False, True):
        seg, pos, alleles, counts = query(sets["random"], rg, sx.prm(2**31 - 1, 1, 0, 1), ss=ss)
        assert seg.tolist() == [0] * (len(rg["rid"]) + 1) and len(pos) == len(alleles) == 0 and counts.shape == ((0, 2, 6) if ss else (0, 6))


def test_refusals_and_the_empty_set(ctx, files, sets):
    _, _, rec, rg, ref = files["random"]
    p = PARAMS[0]
    for kind, r in (("plain", upload(ctx, rec, bases=False)), ("spliced", upload(ctx, rec, bases=False, spliced=True))):
        with pytest.raises(_lib.BsigError, match=f"need reads with bases: a {kind} set") as ei:
            query(r, rg, p)
        assert ei.value.code_name == "BSIG_ERR_ARG"
        r.close()
    reads = sets["random"]
    bad = sx.flat_ref(ref).copy()
    bad[len(bad) // 2] = 5
    with pytest.raises(_lib.BsigError, match="is none of the channel codes 0 .. 4") as ei:
        reads.sites(rg["rid"], rg["loc"], rg["len"], rg["strand"], ref=bad, min_depth=1, min_alt=1, frac=(0, 1))
    assert ei.value.code_name == "BSIG_ERR_ARG"
    for kw, word in ((dict(min_depth=0), "min_depth"), (dict(min_alt=0), "min_alt"), (dict(frac=(2, 1)), "frac_num"), (dict(frac=(0, 0)), "frac_den"),
                     (dict(alt_mask=0), "alt_mask"), (dict(min_base_qual=94), "min_base_qual")):
        with pytest.raises(_lib.BsigError, match=word):
            reads.sites(rg["rid"], rg["loc"], rg["len"], rg["strand"], **kw)
    with pytest.raises(_lib.BsigError, match="reference 3 is not one of the set's 3"):
        query(reads, dict(rid=np.int32([3]), loc=np.int32([0]), len=np.int32([5]), strand=np.int32([0])), p)
    # no range; the empty set
    seg, pos, alleles, counts = query(reads, {k: v[:0] for k, v in rg.items()}, p)
    assert seg.tolist() == [0] and len(pos) == 0
    none = {k: np.zeros(0, dtype=v.dtype) for k, v in rec.items() if k not in ("ref_len", "ref_off")}
    none.update(ref_len=rec["ref_len"], ref_off=np.zeros(len(rec["ref_len"]) + 1, dtype=np.int64),
                cigar_off=np.zeros(1, dtype=np.int64), seq_off=np.zeros(1, dtype=np.int64))
    empty = upload(ctx, none)
    seg, pos, alleles, counts = query(empty, rg, p, ref, ss=True)
    assert seg.tolist() == [0] * (len(rg["rid"]) + 1) and len(pos) == 0 and counts.shape == (0, 2, 6)
    empty.close()


# ---- the file-level call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", ["all", "regions"])
@pytest.mark.parametrize("deck", DECKS)
def test_file_level(files, deck, decode, monkeypatch):
    path, names, _, rg, ref = files[deck]
    monkeypatch.setenv("BAMSIGNALS_DECODE", decode)
    lib = _lib.load()
    lib.bsig_cache_clear()
    gr = nx.granges(names, rg)
    text = ["".join("ACGTN"[c] for c in r) for r in ref]
    assert np.array_equal(ref_codes(text, rg["len"]), sx.flat_ref(ref))
    n_sites = 0
    for k, (ss, kw, with_ref) in enumerate(((False, dict(minDepth=1, minAlt=1, minFraction=0), True),
                                            (True, dict(minDepth=3, minAlt=2, minFraction=0.25, deletions=False, mapqual=30, filteredFlag=0x400,
                                                        minBaseQuality=nx.MINQ), False))):
        got = bamSites(path, gr, ref=text if with_ref else None, ss=ss, verbose=False, **kw)
        route = last_call_route()
        assert "sites" in route and "with bases" in route
        assert bool(last_call_timing()["bam_was_resident"]) == (k > 0), "the second call finds the first one's set: no second decode"
        nuc_kw = {key: kw[key] for key in ("mapqual", "filteredFlag", "minBaseQuality") if key in kw}
        cells = list(bamNucleotides(path, gr, ss=ss, verbose=False, **nuc_kw))
        assert bool(last_call_timing()["bam_was_resident"]), "the nucleotide call uses the same resident set"
        num, den = (0, 1) if k == 0 else (1, 4)
        want = sx.expected_sites(cells, ref if with_ref else None,
                                 sx.prm(kw["minDepth"], kw["minAlt"], num, den, sx.MASK_WITH_DELETIONS if kw.get("deletions", True) else sx.MASK_BASES))
        assert len(got) == len(gr) and got.ss == ss
        assert sx.same_sites((got.seg_off, got.pos, got.base | got.alt << 8, got.counts), want)
        assert not got.pos.flags.writeable
        n_sites += got.nsites
    assert n_sites > 0
    lib.bsig_cache_clear()
