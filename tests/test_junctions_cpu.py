"""CPU: the junctions' expected side (tests/junctions_expected.py: rows with anchors from spliced_expected._intervals, the
per-range result via np.unique) against a brute force; the properties of the deck with planted multiplicities; the Junctions
class from hand-made integers; bamJunctions' own refusals and the parameter rule at file level, none of which needs a device."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import junctions_expected as jx
import spliced_expected as sx

BAM = os.path.join(GOLDEN, "randomBam.bam")
I32 = np.int32


def test_the_package_exports_the_feature():
    import bamsignals_amd
    assert callable(bamsignals_amd.bamJunctions) and isinstance(bamsignals_amd.Junctions, type)
    assert "bamJunctions" in bamsignals_amd.__all__ and "Junctions" in bamsignals_amd.__all__


@pytest.fixture(scope="module")
def hand():
    cols = sx.hand_deck()
    return cols, jx.rows(cols)


def _row(jr, ref, start):
    k = np.flatnonzero((jr["ref"] == ref) & (jr["start"] == start))
    return [(int(jr["end"][i]), int(jr["anchor"][i])) for i in k]


def test_rows_of_the_hand_deck(hand):
    cols, jr = hand
    g = sx.gaps(cols)
    assert len(jr["start"]) == len(g["pos"]) == 35_038 and len(jx.multiplicities(jr)[0]) == 35_037
    assert np.array_equal(np.sort(jr["start"]), np.sort(g["pos"])) and np.array_equal(jr["ref_off"], g["ref_off"])
    assert np.array_equal(np.lexsort((jr["end"], jr["start"], jr["ref"])), np.arange(len(jr["ref"]))), "sorted by (ref, start, end)"
    # (end, anchor) of the rows that start where the case's gap starts
    assert _row(jr, 0, 450) == [(459, 50)]                       # 50M5N5N50M: one gap of 10
    assert _row(jr, 0, 470) == [(479, 50)]                       # 50M5N3I5N50M: the insertion parts nothing
    assert _row(jr, 0, 300) == [(309, 0)]                        # 10N90M: nothing on the left
    assert _row(jr, 0, 410) == [(419, 0)]                        # 90M10N: nothing on the right
    assert _row(jr, 0, 600) == [(799, 0)]                        # 200N
    assert not np.any((jr["ref"] == 0) & (jr["start"] == 670))   # flag 4: no row
    assert _row(jr, 0, 590) == [(639, 40)]                       # 30M10D30M50N40M: left 70, right 40
    assert _row(jr, 0, 9) == [(28, 10)]                          # the read at pos -1
    assert _row(jr, 0, 1110) == [(1119, 10)]                     # 10M5N0M5N85M: an operation of length 0 parts nothing
    assert _row(jr, 0, 1200) == [(1209, 0)] and _row(jr, 0, 1300) == [(1309, 0)]     # 3S10N4I90M2P10N opens and closes with a gap


def _hand_ranges():
    rid = [0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 1, 0]
    loc = [0, 140, 450, 451, 0, 1_000_000, 2_999_000, 0, 100_000, 990, 0, 500]
    ln = [5000, 2100, 13, 12, 0, 1_100_000, 1_200, 3000, 70_001, 1100, 5000, 200]
    strand = [1, -1, 0, 1, -1, 0, 1, -1, 0, 1, -1, -1]
    return dict(rid=np.asarray(rid, I32), loc=np.asarray(loc, I32), len=np.asarray(ln, I32), strand=np.asarray(strand, I32))


@pytest.mark.parametrize("ss", [False, True])
@pytest.mark.parametrize("flt", [dict(), dict(mapqual=30, filteredF=0x400), dict(min_anchor=1), dict(min_anchor=8),
                                 dict(mapqual=30, filteredF=0x400, min_anchor=51), dict(requiredF=16)])
def test_restatement_is_the_brute_force(hand, ss, flt):
    _, jr = hand
    rg = _hand_ranges()
    want = jx.brute(jr, rg, ss=ss, **flt)
    got = jx.expected(jr, rg, ss=ss, **flt)
    assert jx.same(got, want)
    if not flt:
        assert want[0][-1] > 35_000 and want[0][5] == want[0][4], "the long read's junctions; a width-0 range owns nothing"
        i = int(want[0][2])
        assert (want[1][i], want[2][i]) == (450, 459) and want[0][3] - want[0][2] == 1 and want[0][4] - want[0][3] == 0, \
                "loc = start holds the junction, loc = start + 1 does not"


def test_deck_properties():
    cols = jx.junction_deck()
    assert list(cols["ref_len"]) == [500_000, 5_000, 500_000] and cols["ref_off"][1] == cols["ref_off"][2]
    assert len(cols["pos"]) == 2 * sum(jx.READS_PER_GENE)
    jr = jx.rows(cols)
    u, c = jx.multiplicities(jr)
    assert c.max() >= 1024, "four workgroups of 256"
    assert np.count_nonzero(c >= 257) >= 5 and np.count_nonzero(c == 1) >= 10
    ends_per_start = np.unique(u[:, :2], axis=0, return_counts=True)[1]
    starts_per_end = np.unique(u[:, [0, 2]], axis=0, return_counts=True)[1]
    assert np.count_nonzero(ends_per_start > 1) >= 20 and np.count_nonzero(starts_per_end > 1) >= 20
    assert 0.05 <= np.mean(jr["anchor"] < 8) <= 0.30
    assert jr["anchor"].max() <= 50, "reads of 100 bases: at min_anchor = 51 nothing is left"
    assert jr["start"].min() >= 0 and np.all(jr["end"] < np.asarray(cols["ref_len"])[jr["ref"]]), "every gap inside its reference"
    assert set(np.unique(jr["mapq"]).tolist()) == {0, 3, 30, 60} and 0 < np.mean((jr["flag"] & 0x400) != 0) < 0.1
    g = jx.junction_genes()
    assert len(g["rid"]) == 20 and set(g["strand"].tolist()) == {-1, 1}
    # a start that exactly one row has: what the GPU suite repeats to place a run at a chosen work item
    assert np.count_nonzero(np.unique(np.stack([jr["ref"], jr["start"]], axis=1), axis=0, return_counts=True)[1] == 1) >= 1


# ---- the Junctions class ----------------------------------------------------------------------------------------------------
def _made(ss):
    from bamsignals_amd import Junctions
    count = [[3, 1], [0, 2], [5, 5], [1, 0]] if ss else [4, 2, 10, 1]
    return Junctions([0, 2, 2, 4], [101, 101, 40, 60], [200, 300, 80, 70], count, [50, 7, 12, 0], ss)


def test_junctions_class():
    from bamsignals_amd import GRanges, Junctions
    j = _made(False)
    assert len(j) == 3 and j.njunctions == 4 and "3 ranges, 4 junctions" in repr(j)
    assert j.count.dtype == np.int64 and j.count.shape == (4,) and _made(True).count.shape == (4, 2)
    assert j[0]["start"].tolist() == [101, 101] and j[0]["end"].tolist() == [200, 300] and j[0]["count"].tolist() == [4, 2]
    assert len(j[1]["start"]) == 0 and j[-1]["max_anchor"].tolist() == [12, 0] and len(list(j)) == 3
    with pytest.raises(IndexError):
        j[3]
    with pytest.raises(TypeError):
        j["a"]
    for a in (j.seg_off, j.start, j.end, j.count, j.max_anchor):
        with pytest.raises(ValueError):
            a[...] = 0
    k = j.with_support(4)
    assert k.seg_off.tolist() == [0, 1, 1, 2] and k.start.tolist() == [101, 40] and k.count.tolist() == [4, 10]
    ks = _made(True).with_support(4)
    assert ks.seg_off.tolist() == [0, 1, 1, 2] and ks.count.tolist() == [[3, 1], [5, 5]]
    gr = GRanges(["chr1", "chr2", "chr2"], [1, 1, 30], width=[1000, 10, 100], strand=["+", "*", "-"])
    out, colsd = j.to_granges(gr)
    assert list(out.seqnames) == ["chr1", "chr1", "chr2", "chr2"] and list(out.strand) == ["+", "+", "-", "-"]
    assert out.start.tolist() == [101, 101, 40, 60] and out.width.tolist() == [100, 200, 41, 11], "a '-' range mirrors nothing"
    assert colsd["range"].tolist() == [0, 0, 2, 2] and colsd["count"].tolist() == [4, 2, 10, 1]
    with pytest.raises(ValueError):
        j.to_granges(gr[:2])
    for bad in (dict(seg_off=[0, 2, 2, 3]), dict(seg_off=[1, 2, 2, 4]), dict(end=[200, 300, 80, 59]), dict(count=[4, 2, 10]),
                dict(count=[4, 2, -1, 1]), dict(ss=1)):
        a = dict(seg_off=[0, 2, 2, 4], start=[101, 101, 40, 60], end=[200, 300, 80, 70], count=[4, 2, 10, 1], max_anchor=[50, 7, 12, 0],
                 ss=False)
        a.update(bad)
        with pytest.raises(ValueError):
            Junctions(**a)


def test_bed_text(tmp_path):
    from bamsignals_amd import GRanges
    gr = GRanges(["chr1", "chr2", "chr2"], [1, 1, 30], width=[1000, 10, 100], strand=["+", "*", "-"])
    p = str(tmp_path / "j.bed")
    assert _made(False).to_bed(p, gr) == 4
    assert open(p).read() == ("chr1\t100\t200\trange0_0\t4\t.\nchr1\t100\t300\trange0_1\t2\t.\n"
                              "chr2\t39\t80\trange2_0\t10\t.\nchr2\t59\t70\trange2_1\t1\t.\n")
    assert _made(True).to_bed(p, gr) == 4
    # sense of a '+' range is '+', of a '-' range '-'; the stronger strand, a tie to sense
    assert open(p).read() == ("chr1\t100\t200\trange0_0\t4\t+\nchr1\t100\t300\trange0_1\t2\t-\n"
                              "chr2\t39\t80\trange2_0\t10\t-\nchr2\t59\t70\trange2_1\t1\t-\n")


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_bamjunctions_refuses_bad_arguments_before_any_native_call(monkeypatch):
    from bamsignals_amd import GRanges, _lib, bamJunctions

    def no_native(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_lib, "load", no_native)
    gr = GRanges(["chr1"], [1], width=[100])
    for kw, words in ((dict(mapqual=-1), "mapqual"), (dict(mapqual=256), "mapqual"), (dict(mapqual=1.5), "mapqual"),
                      (dict(mapqual=True), "mapqual"), (dict(filteredFlag="x"), "filteredFlag"), (dict(filteredFlag=1 << 16), "filteredFlag"),
                      (dict(minAnchor=-1), "minAnchor"), (dict(minAnchor=2.0), "minAnchor"), (dict(minAnchor=1 << 31), "minAnchor"),
                      (dict(ss=1), "ss must be True or False")):
        with pytest.raises(ValueError, match=words):
            bamJunctions(BAM, gr, verbose=False, **kw)
    with pytest.raises(TypeError, match="GRanges"):
        bamJunctions(BAM, [("chr1", 1, 100)], verbose=False)


def _call(min_anchor=0, width=(100, 100), result=True, path=BAM, level2=b"chr2"):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray(width, I32)
    codes, start, strand = np.arange(2, dtype=I32), np.full(2, 1000, I32), np.ones(2, I32)
    levels = (C.c_char_p * 2)(b"chr1", level2)
    h = C.c_void_p()
    rc = lib.bsig_junctions(path.encode(), 2, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
                            0, 0, -1, min_anchor, 0, -1, C.byref(h) if result else None)
    assert not h.value                                   # (a refused call hands out nothing)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


MISSING = os.path.join(GOLDEN, "no_such_file.bam")


@pytest.mark.parametrize("a, want", [
    (dict(min_anchor=-1), (-1, "min_anchor must not be negative (-1 given)")),
    (dict(min_anchor=-1, path=MISSING), (-1, "min_anchor must not be negative (-1 given)")),
    (dict(width=(100, -5)), (-1, "range 1 has a negative width")),
    (dict(width=(100, -5), path=MISSING), (-1, "range 1 has a negative width")),
    (dict(result=False), (-1, "result is NULL")),
    (dict(result=False, path=MISSING), (-1, "result is NULL")),
    (dict(path=MISSING), (-2, "Fail to open BAM file <missing>")),
    (dict(level2=b"chrNone"), (-4, "chromosome chrNone not present in the bam file")),
])
def test_parameter_rule_at_file_level(a, want):
    rc, msg, route = _call(**a)
    assert (rc, msg.replace(MISSING, "<missing>")) == want
    assert route == b""                                  # refused: before the BAM is opened where the parameters are at fault
