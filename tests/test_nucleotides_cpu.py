"""CPU: the restatement of bamNucleotides against a second one that shares no code with it, the independent BAM reader against
what was written, the invariant that ties the counts to bamCoverage(splice=True), the host maker of the base columns against
the independent reader, the parameter refusals of bamNucleotides and NucleotideCounts' methods.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import nucleotides_expected as nx
import spliced_expected as sx
from bamsignals_amd import GRanges, NucleotideCounts, _lib, bamNucleotides
from bamsignals_amd.bamio import _view

PARAMS = (dict(), dict(ss=True, min_base_qual=nx.MINQ), dict(ss=True, mapqual=30, filteredF=0x400, min_base_qual=93),
          dict(requiredF=16, min_base_qual=1))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("nucleotides_cpu")
    out = {}
    for name, names, (rec, rg) in (("hand", nx.HAND_NAMES, nx.hand_deck()), ("random", nx.RANDOM_NAMES, nx.random_deck())):
        out[name] = (nx.write_bam(d / f"{name}.bam", names, rec), names, rec, rg)
    path, rg = nx.write_real_deck(d / "real.bam", n=20_000)
    out["real"] = (path, nx.REAL_NAMES, None, rg)
    return out


@pytest.mark.parametrize("deck", ["hand", "random"])
def test_expected_is_brute(deck):
    rec, rg = nx.hand_deck() if deck == "hand" else nx.random_deck()
    seen = 0
    for kw in PARAMS:
        e, b = nx.expected(rec, rg, **kw), nx.brute(rec, rg, **kw)
        assert nx.same(e, b), kw
        seen += sum(int(a.sum()) for a in e)
    assert seen > 0


def test_expected_is_brute_on_real_shaped_records(files):
    """20,000 real-shaped records here, not the GPU suite's 200,000: `brute` visits every base of every read in Python"""
    path, _, _, rg = files["real"]
    names, rec = nx.read_bam(path)
    assert names == nx.REAL_NAMES and len(rec["pos"]) == 20_000 and np.all(np.diff(rec["seq_off"]) == 100)
    for kw in PARAMS[:3]:
        assert nx.same(nx.expected(rec, rg, **kw), nx.brute(rec, rg, **kw)), kw


@pytest.mark.parametrize("deck", ["hand", "random"])
def test_the_reader_returns_what_was_written(files, deck):
    path, names, rec, _ = files[deck]
    got_names, got = nx.read_bam(path)
    assert got_names == names
    for k in rec:
        assert got[k].dtype == rec[k].dtype and np.array_equal(got[k], rec[k]), k
    if deck == "hand":
        assert np.diff(rec["cigar_off"]).max() == nx.LONG_OPS, "the CG tag's CIGAR, not the placeholder"


@pytest.mark.parametrize("deck", ["random", "hand"])
def test_channels_add_up_to_the_spliced_coverage(deck):
    """min_base_qual 0: A + C + G + T + N + '-' at a base is the coverage of the reads' blocks there (D covered, N not), for
    reads that take part and have a reference-consuming operation (the hand deck: those reads only)"""
    rec, rg = nx.hand_deck() if deck == "hand" else nx.random_deck()
    moves = np.isin(rec["cigar"] & 0xF, (0, 2, 3, 7, 8)) & (rec["cigar"] >> 4 > 0)
    per_read = np.add.reduceat(np.concatenate([moves, [False]]).astype(np.int64), rec["cigar_off"][:-1]) * (np.diff(rec["cigar_off"]) > 0)
    keep = np.flatnonzero((per_read > 0) & ((rec["flag"] & 4) == 0))
    assert deck == "hand" or len(keep) == len(rec["pos"])
    sub = nx.take(rec, keep)
    rows = sx.blocks(sub)
    for flt in (dict(), dict(mapqual=30, filteredF=0x400)):
        got = nx.expected(sub, rg, **flt)
        for i in range(len(rg["rid"])):
            lo, w = int(rg["loc"][i]), int(rg["len"][i])
            cov = np.zeros(w, dtype=np.int64)
            r0, r1 = rows["ref_off"][rg["rid"][i]], rows["ref_off"][rg["rid"][i] + 1]
            for s, e, f, m in zip(rows["pos"][r0:r1], rows["end"][r0:r1], rows["flag"][r0:r1], rows["mapq"][r0:r1]):
                if nx.takes_part(int(f), int(m), **flt) and e >= lo and s < lo + w:
                    cov[max(int(s) - lo, 0):min(int(e) + 1 - lo, w)] += 1
            assert np.array_equal(got[i].sum(axis=0), cov[::-1] if rg["strand"][i] < 0 else cov), (i, flt)


def decode_bases(path, regions=None):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.bsig_bam_open(str(path).encode(), C.byref(h)))
    cols, bc = _lib.Columns(), _lib.BaseColumns()
    try:
        if regions is None:
            _lib.check(lib.bsig_bam_decode_bases(h, -1, None, None, None, 2, C.byref(cols), C.byref(bc)))
        else:
            rid, beg, end = (np.ascontiguousarray(a, dtype=t) for a, t in zip(regions, (np.int32, np.int64, np.int64)))
            _lib.check(lib.bsig_bam_decode_bases(h, len(rid), rid.ctypes.data, beg.ctypes.data, end.ctypes.data, 2, C.byref(cols), C.byref(bc)))
        n = cols.n_reads
        out = dict(pos=_view(cols.pos, n, np.int32), flag=_view(cols.flag, n, np.uint16), cigar_off=_view(cols.cigar_off, n + 1, np.int64),
                   ref_off=_view(cols.ref_off, cols.n_ref + 1, np.int64), seq_off=_view(bc.seq_off, n + 1, np.int64))
        total = int(out["seq_off"][-1]) if n else 0
        out.update(cigar=_view(cols.cigar, int(out["cigar_off"][-1]) if n else 0, np.uint32), seq=_view(bc.seq, (total + 1) // 2, np.uint8),
                   qual=_view(bc.qual, total, np.uint8))
        return out
    finally:
        lib.bsig_bam_close(h)


@pytest.mark.parametrize("deck", ["hand", "random", "real"])
def test_host_base_columns_are_the_readers(files, deck):
    """bsig_bam_decode_bases, whole and through the index, against the independent reader: offsets, nibbles tightly packed across
    reads of odd length, qualities"""
    path = files[deck][0]
    rec = nx.read_bam(path)[1]
    got = decode_bases(path)
    for k in ("pos", "flag", "ref_off", "cigar_off", "cigar", "seq_off", "qual"):
        assert np.array_equal(got[k], rec[k]), k
    assert np.array_equal(got["seq"], nx.packed(rec))
    assert deck == "real" or np.any(np.diff(rec["seq_off"]) % 2 == 1)
    # index-driven: a superset of the reads that overlap the regions, each once, in file order -- found by (pos, flag, CIGAR, bases)
    regions = ([0, 0], [100, 3000], [900, 5000])
    some = decode_bases(path, regions)
    assert 0 < len(some["pos"]) <= len(rec["pos"])
    first = int(np.searchsorted(rec["pos"][:rec["ref_off"][1]], some["pos"][0]))
    while not (rec["flag"][first] == some["flag"][0] and rec["seq_off"][first + 1] - rec["seq_off"][first] == some["seq_off"][1]):
        first += 1
    part = nx.take(rec, np.arange(first, first + len(some["pos"])))
    for k in ("pos", "flag", "cigar", "seq_off", "qual"):
        assert np.array_equal(some[k], part[k]), k
    assert np.array_equal(some["seq"], nx.packed(part))


def test_parameter_refusals(files):
    path, names, _, rg = files["random"]
    gr = nx.granges(names, rg)
    for kw, word in ((dict(minBaseQuality=94), "minBaseQuality"), (dict(minBaseQuality=-1), "minBaseQuality"), (dict(minBaseQuality=20.0), "minBaseQuality"),
                     (dict(minBaseQuality=True), "minBaseQuality"), (dict(mapqual=256), "mapqual"), (dict(mapqual="3"), "mapqual"),
                     (dict(filteredFlag=0x10000), "filteredFlag"), (dict(filteredFlag=-2), "filteredFlag"), (dict(ss=1), "ss")):
        with pytest.raises(ValueError, match=word):
            bamNucleotides(path, gr, verbose=False, **kw)
    with pytest.raises(TypeError, match="GRanges"):
        bamNucleotides(path, [("r1", 1, 10)], verbose=False)
    # the library judges its own parameter before it opens anything
    lib = _lib.load()
    out = np.zeros(8, dtype=np.int32)
    rc = lib.bsig_nucleotides(b"/nonexistent/no.bam", 0, None, 0, None, None, None, None, 0, 0, -1, 94, 0, -1, out.ctypes.data)
    assert _lib.ERR_NAMES[rc] == "BSIG_ERR_ARG" and b"min_base_qual must lie between 0 and 93" in lib.bsig_last_error()
    rc = lib.bsig_nucleotides(b"/nonexistent/no.bam", 0, None, 0, None, None, None, None, 0, 0, -1, 93, 0, -1, out.ctypes.data)
    assert _lib.ERR_NAMES[rc] == "BSIG_ERR_IO"


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("bsig_reads_upload_bases", "bsig_reads_has_bases", "bsig_reads_base_table_bytes", "bsig_bam_decode_bases",
                 "bsig_reads_from_bam_bases", "bsig_reads_from_bam_regions_bases", "bsig_nucleotides_cells", "bsig_reads_nucleotides",
                 "bsig_reads_nucleotides_host", "bsig_nucleotides"):
        assert hasattr(lib, name), name
    ln = np.asarray([5, 0, 7], dtype=np.int32)
    off = np.zeros(4, dtype=np.int64)
    assert lib.bsig_nucleotides_cells(3, ln.ctypes.data, 0, off.ctypes.data) == 72 and off.tolist() == [0, 30, 30, 72]
    assert lib.bsig_nucleotides_cells(3, ln.ctypes.data, 1, off.ctypes.data) == 144 and off.tolist() == [0, 60, 60, 144]
    assert lib.bsig_nucleotides_cells(1, np.asarray([-1], dtype=np.int32).ctypes.data, 0, None) == -1
    assert lib.bsig_reads_has_bases(None) == 0 and lib.bsig_reads_base_table_bytes(None) == 0


def test_nucleotide_counts_methods():
    a = np.zeros((6, 5), dtype=np.int32)
    a[:, 0] = [3, 1, 0, 0, 0, 0]        # A wins
    a[:, 1] = [2, 2, 0, 0, 0, 1]        # a tie: the first
    a[:, 3] = [0, 0, 0, 0, 1, 4]        # deletions win
    a[:, 4] = [0, 0, 0, 7, 0, 0]
    b = np.zeros((6, 0), dtype=np.int32)
    nc = NucleotideCounts([a, b])
    assert len(nc) == 2 and nc.channels == ("A", "C", "G", "T", "N", "-") and not nc.ss
    assert nc[0].shape == (6, 5) and nc[-1].shape == (6, 0) and not nc[0].flags.writeable
    assert nc.depth(0).tolist() == [4, 5, 0, 5, 7] and nc.depth(0).dtype == np.int64
    assert nc.major(0).tolist() == [0, 0, -1, 5, 3] and nc.major(1).tolist() == []
    f = nc.fraction(0, "A")
    assert f.dtype == np.float64 and f[0] == 0.75 and f[1] == 0.4 and np.isnan(f[2]) and f[4] == 0.0
    assert nc.fraction(0, 5)[3] == 0.8
    gr = GRanges(["c1", "c2"], [101, 7], width=[5, 0], strand=["-", "+"])
    t = nc.to_table(gr)
    assert t["seqnames"] == ["c1"] * 4 and t["pos"].tolist() == [105, 104, 102, 101] and t["range"].tolist() == [0] * 4
    assert t["A"].tolist() == [3, 2, 0, 0] and t["-"].tolist() == [0, 1, 4, 0] and t["T"].tolist() == [0, 0, 0, 7]
    both = NucleotideCounts([np.stack([a, 2 * a])], ss=True)
    assert both[0].shape == (2, 6, 5) and both.depth(0).tolist() == [12, 15, 0, 15, 21] and both.major(0).tolist() == [0, 0, -1, 5, 3]
    with pytest.raises(ValueError):
        NucleotideCounts([a], ss=True)
    with pytest.raises(ValueError):
        NucleotideCounts([a.astype(np.int64)])
    with pytest.raises(IndexError):
        nc[2]
    with pytest.raises(TypeError):
        nc["0"]
    with pytest.raises(ValueError):
        nc.to_table(gr[0])
    with pytest.raises(ValueError):
        nc.fraction(0, "U")
