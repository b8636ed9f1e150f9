"""GPU: the base table of reads with bases and the nucleotide counts at handle level (Reads.nucleotides) and at file level
(bamNucleotides), against tests/nucleotides_expected.py: the plain restatement of the walk.  Expectations of files come from
that module's own BAM reader, never from the library's decode.  All results are integers and compared exactly."""
import itertools

import numpy as np
import pytest

import nucleotides_expected as nx
from bamsignals_amd import BamFile, _lib, bamCoverage, bamNucleotides
from bamsignals_amd.device import Context, Plan, Reads, make_params
from bamsignals_amd.wrappers import last_call_route, last_call_timing

pytestmark = pytest.mark.gpu

FILTERS = (dict(), dict(mapqual=30, filteredF=0x400))
QUALS = (0, nx.MINQ, 93)
DECKS = ("hand", "random", "real")


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
    """name -> (path, names, the records the independent reader finds in the file, ranges): written once, left unchanged"""
    d = tmp_path_factory.mktemp("nucleotides")
    out = {}
    for name, names, (rec, rg) in (("hand", nx.HAND_NAMES, nx.hand_deck()), ("random", nx.RANDOM_NAMES, nx.random_deck())):
        path = nx.write_bam(d / f"{name}.bam", names, rec)
        out[name] = (path, names, nx.read_bam(path)[1], rg)
    path, rg = nx.write_real_deck(d / "real.bam")
    out["real"] = (path, nx.REAL_NAMES, nx.read_bam(path)[1], rg)
    return out


@pytest.fixture(scope="module")
def sets(ctx, files):
    """name -> the resident set with bases, uploaded from the reader's records"""
    out = {name: upload(ctx, rec) for name, (_, _, rec, _) in files.items()}
    yield out
    for r in out.values():
        r.close()


_wanted = {}


def want(files, deck, ss, min_base_qual=0, **flt):
    """the restatement on the deck's own ranges, computed once per parameter set (with ss; without it the two planes add up)"""
    key = (deck, min_base_qual, tuple(sorted(flt.items())))
    if key not in _wanted:
        _, _, rec, rg = files[deck]
        _wanted[key] = nx.expected(rec, rg, ss=True, min_base_qual=min_base_qual, **flt)
    return _wanted[key] if ss else [a.sum(axis=0, dtype=np.int32) for a in _wanted[key]]


def query(reads, rg, **kw):
    return reads.nucleotides(rg["rid"], rg["loc"], rg["len"], rg["strand"], **kw)


# ---- the query == the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck", DECKS)
def test_uploaded_bases_give_the_restatement(files, sets, deck):
    reads, rg = sets[deck], files[deck][3]
    assert reads.has_bases and not reads.spliced
    total = 0
    for ss, flt, q in itertools.product((False, True), FILTERS, QUALS):
        got = query(reads, rg, ss=ss, min_base_qual=q, **flt)
        exp = want(files, deck, ss, q, **flt)
        assert nx.same(got, exp), (ss, flt, q)
        assert all(a.dtype == np.int32 and a.shape == ((2, 6, w) if ss else (6, w)) for a, w in zip(got, rg["len"]))
        total += sum(int(a.sum()) for a in got)
    assert total > 0


@pytest.mark.parametrize("deck", ["hand", "random"])
def test_ranges_reversed_and_twice(files, sets, deck):
    reads, rg = sets[deck], files[deck][3]
    n = len(rg["rid"])
    order = np.concatenate([np.arange(n)[::-1], np.arange(n)])
    twice = {k: v[order] for k, v in rg.items()}
    for ss, q in ((False, 0), (True, nx.MINQ)):
        exp = want(files, deck, ss, q)
        got = query(reads, twice, ss=ss, min_base_qual=q)
        assert nx.same(got, [exp[i] for i in order])
        assert nx.same(query(reads, twice, ss=ss, min_base_qual=q), got), "a second run gives the same cells"


def test_planted_cells(files, sets):
    """what the hand deck plants, read off the result itself"""
    reads = sets["hand"]
    rg = dict(rid=np.int32([0, 0, 0]), loc=np.int32([4000, 4000, 100]), len=np.int32([3, 3, 16]), strand=np.int32([1, -1, 1]))
    plus, minus, codes = query(reads, rg)
    assert plus[:, 0].tolist() == [70_000, 0, 0, 0, 0, 0] and plus[:, 1].tolist() == [0, 70_000, 0, 0, 0, 0]     # A, C, T: past 16 bits
    assert plus[:, 2].tolist() == [0, 0, 0, 70_000, 0, 0]
    assert minus[:, 0].tolist() == [70_000, 0, 0, 0, 0, 0] and minus[:, 2].tolist() == [0, 0, 0, 70_000, 0, 0]  # T -> A first, A -> T last
    # the two reads that spell every code, one forwards and one backwards: position j shows code j and code 15 - j
    ch = [nx._CHANNEL_OF_CODE[j] for j in range(16)]
    for j in range(16):
        assert codes[ch[j], j] >= 1 and codes[ch[15 - j], j] >= 1


# ---- decoded from the file: whole and index-driven -----------------------------------------------------------------------------
@pytest.mark.parametrize("device_decode", ["require", "0"])
@pytest.mark.parametrize("deck", DECKS)
def test_decoded_from_the_file(ctx, files, deck, device_decode, monkeypatch):
    """both decode routes: the bases copied out of the inflated stream on the GPU ("require": no silent change of path), and the
    CPU fallback's columns through the upload"""
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", device_decode)
    path, _, rec, rg = files[deck]
    bam = BamFile(path)
    whole = Reads.from_bam(ctx, bam, bases=True)
    some = Reads.from_bam_regions(ctx, bam, rg["rid"], rg["loc"].astype(np.int64), rg["loc"].astype(np.int64) + rg["len"], bases=True)
    assert whole.has_bases and some.has_bases and whole.info()["n_reads"] == len(rec["pos"]) >= some.info()["n_reads"]
    assert whole.base_table_bytes == table_bytes(rec)
    for reads in (whole, some):
        for ss, flt, q in ((False, FILTERS[0], 0), (True, FILTERS[1], nx.MINQ)):
            assert nx.same(query(reads, rg, ss=ss, min_base_qual=q, **flt), want(files, deck, ss, q, **flt)), (ss, flt, q)
        reads.close()
    bam.close()


def table_bytes(rec):
    n, n_ops, n_bases, n_ref = len(rec["pos"]), len(rec["cigar"]), len(rec["code"]), len(rec["ref_len"])
    return 28 * n + 16 + 4 * n_ops + (n_bases + 1) // 2 + n_bases + 8 * (n_ref + 1)


@pytest.mark.parametrize("chunk_mb", [None, "1"])
def test_several_chunks_inflated_on_the_gpu(ctx, files, monkeypatch, chunk_mb):
    """the real-shaped deck (21 MB of BAM, 40 MB of stream) in chunks of 1 MB, inflated on the GPU: every chunk leaves its piece
    of the base table, and the pieces that begin on an odd nibble are shifted into place; beside it the same file in one chunk"""
    path, names, rec, rg = files["real"]
    monkeypatch.setenv("BAMSIGNALS_INFLATE", "gpu")
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", "require")
    if chunk_mb:
        monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE_CHUNK_MB", chunk_mb)
    bam = BamFile(path)
    whole = Reads.from_bam(ctx, bam, bases=True)
    some = Reads.from_bam_regions(ctx, bam, rg["rid"], rg["loc"].astype(np.int64), rg["loc"].astype(np.int64) + rg["len"], bases=True)
    assert whole.base_table_bytes == table_bytes(rec) and whole.info()["n_reads"] == len(rec["pos"]) > some.info()["n_reads"] > 0
    for reads in (whole, some):
        for ss, flt, q in ((False, FILTERS[0], 0), (True, FILTERS[1], nx.MINQ), (True, FILTERS[0], 93)):
            assert nx.same(query(reads, rg, ss=ss, min_base_qual=q, **flt), want(files, "real", ss, q, **flt)), (ss, flt, q)
        reads.close()
    bam.close()
    monkeypatch.setenv("BAMSIGNALS_DECODE", "all")
    lib = _lib.load()
    lib.bsig_cache_clear()
    got = bamNucleotides(path, nx.granges(names, rg), ss=True, minBaseQuality=nx.MINQ, verbose=False)
    assert nx.same(list(got), want(files, "real", True, nx.MINQ))
    lib.bsig_cache_clear()


def test_an_odd_deck_in_small_chunks(ctx, tmp_path, monkeypatch):
    """reads of 1 .. 41 bases, odd and even, in 1-MB chunks: every chunk's nibble total is as likely odd as even"""
    rng = np.random.default_rng(11)
    n = 60_000
    pos = np.sort(rng.integers(0, 50_000, n))
    ln = rng.integers(1, 42, n)
    rec = nx.columns([60_000], np.zeros(n), pos, np.where(rng.random(n) < 0.5, 16, 0), np.full(n, 30), np.zeros(n), [[int(x) << 4] for x in ln],
                     [rng.choice([1, 2, 4, 8, 15], int(x)).astype(np.uint8) for x in ln], [rng.integers(10, 41, int(x)).astype(np.uint8) for x in ln])
    path = nx.write_bam(tmp_path / "odd.bam", ["c"], rec)
    rg = dict(rid=np.int32([0, 0]), loc=np.int32([0, 20_000]), len=np.int32([60_000, 3_000]), strand=np.int32([1, -1]))
    exp = nx.expected(rec, rg, ss=True, min_base_qual=25)
    monkeypatch.setenv("BAMSIGNALS_INFLATE", "gpu")
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", "require")
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE_CHUNK_MB", "1")
    bam = BamFile(path)
    reads = Reads.from_bam(ctx, bam, bases=True)
    assert reads.base_table_bytes == table_bytes(rec)
    assert nx.same(query(reads, rg, ss=True, min_base_qual=25), exp)
    reads.close()
    bam.close()


@pytest.mark.parametrize("device_decode", ["require", "0"])
@pytest.mark.parametrize("decode", ["all", "regions"])
@pytest.mark.parametrize("deck", DECKS)
def test_file_level(files, deck, decode, device_decode, monkeypatch):
    path, names, _, rg = files[deck]
    monkeypatch.setenv("BAMSIGNALS_DECODE", decode)
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", device_decode)
    lib = _lib.load()
    lib.bsig_cache_clear()
    gr = nx.granges(names, rg)
    for k, (ss, kw, flt, q) in enumerate(((False, dict(), dict(), 0),
                                           (True, dict(mapqual=30, filteredFlag=0x400, minBaseQuality=nx.MINQ), FILTERS[1], nx.MINQ))):
        got = bamNucleotides(path, gr, ss=ss, verbose=False, **kw)
        route = last_call_route()
        assert "nucleotides" in route and "with bases" in route
        assert bool(last_call_timing()["bam_was_resident"]) == (k > 0), "the second call finds the first one's set: no second decode"
        assert len(got) == len(gr) and got.channels == ("A", "C", "G", "T", "N", "-")
        assert nx.same(list(got), want(files, deck, ss, q, **flt))
        assert not got[0].flags.writeable
    lib.bsig_cache_clear()


def test_depth_is_the_spliced_coverage(files):
    """minBaseQuality 0: the six channels of a base add up to bamCoverage(splice=True) there (D covered, N not)"""
    path, names, _, rg = files["random"]
    gr = nx.granges(names, rg)
    lib = _lib.load()
    lib.bsig_cache_clear()
    for kw in (dict(), dict(mapqual=30, filteredFlag=0x400)):
        nuc = bamNucleotides(path, gr, verbose=False, **kw)
        cov = bamCoverage(path, gr, verbose=False, splice=True, **kw)
        assert "spliced" in last_call_route() and "with bases" not in last_call_route()
        assert all(np.array_equal(nuc.depth(i), np.asarray(cov[i], dtype=np.int64)) for i in range(len(gr)))
        assert sum(int(nuc.depth(i).sum()) for i in range(len(gr))) > 0
    lib.bsig_cache_clear()


# ---- the set ------------------------------------------------------------------------------------------------------------------
def test_a_set_with_bases_is_a_plain_set(ctx, files, sets):
    _, _, rec, rg = files["real"]
    with_bases = sets["real"]
    plain = upload(ctx, rec, bases=False)
    clone = with_bases.clone(ctx)
    assert clone.has_bases and not plain.has_bases and plain.base_table_bytes == 0
    for mode, args in ((_lib.MODE_COVERAGE, dict()), (_lib.MODE_PROFILE, dict(binsize=1, ss=True, shift=10)), (_lib.MODE_COUNT, dict(binsize=-1))):
        res = []
        for r in (plain, with_bases, clone):
            plan = Plan(ctx, r, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(mode, **args))
            res.append(plan.run_host().copy())
            plan.close()
        assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2]) and res[0].sum() > 0
    assert nx.same(query(clone, rg, ss=True, min_base_qual=nx.MINQ), want(files, "real", True, nx.MINQ))
    # hbm_bytes grows by the table's stated size: every array of this table is a block of its own but the reference offsets,
    # and a cached block may be an eighth larger than asked
    stated = with_bases.base_table_bytes
    assert stated == clone.base_table_bytes == table_bytes(rec)
    for r in (with_bases, clone):
        grown = r.info()["hbm_bytes"] - plain.info()["hbm_bytes"]
        assert stated - 4096 <= grown <= stated * 1.125 + (4 << 20), (grown, stated)
    with pytest.raises(_lib.BsigError, match="reads with bases have no reads file") as ei:
        with_bases.save("/nonexistent/never_written.bsig")
    assert ei.value.code_name == "BSIG_ERR_ARG"
    plain.close()
    clone.close()


def test_refusals_and_the_empty_set(ctx, files, sets):
    _, _, rec, rg = files["random"]
    for kind, r in (("plain", upload(ctx, rec, bases=False)), ("spliced", upload(ctx, rec, bases=False, spliced=True))):
        assert not r.has_bases
        with pytest.raises(_lib.BsigError, match=f"need reads with bases: a {kind} set") as ei:
            query(r, rg)
        assert ei.value.code_name == "BSIG_ERR_ARG"
        r.close()
    reads = sets["random"]
    for bad in (94, -1):
        with pytest.raises(_lib.BsigError, match="min_base_qual must lie between 0 and 93") as ei:
            query(reads, rg, min_base_qual=bad)
        assert ei.value.code_name == "BSIG_ERR_ARG"
    with pytest.raises(_lib.BsigError, match="reference 3 is not one of the set's 3"):
        query(reads, dict(rid=np.int32([3]), loc=np.int32([0]), len=np.int32([5]), strand=np.int32([0])))
    with pytest.raises(_lib.BsigError, match="min_base_qual must lie between 0 and 93"):
        lib = _lib.load()
        out = np.zeros(8, dtype=np.int32)
        _lib.check(lib.bsig_nucleotides(b"/nonexistent/no.bam", 0, None, 0, None, None, None, None, 0, 0, -1, 94, 0, -1, out.ctypes.data))
    none = {k: np.zeros(0, dtype=v.dtype) for k, v in rec.items() if k not in ("ref_len", "ref_off")}
    none.update(ref_len=rec["ref_len"], ref_off=np.zeros(len(rec["ref_len"]) + 1, dtype=np.int64),
                cigar_off=np.zeros(1, dtype=np.int64), seq_off=np.zeros(1, dtype=np.int64))
    empty = upload(ctx, none)
    assert empty.has_bases and empty.base_table_bytes == 0
    got = query(empty, rg, ss=True)
    assert all(a.shape == (2, 6, w) and not a.any() for a, w in zip(got, rg["len"]))
    assert query(reads, {k: v[:0] for k, v in rg.items()}) == []
    empty.close()
