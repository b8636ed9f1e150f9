"""CPU: bamCoverage(splice=True) -- the semantics restated in numpy (tests/spliced_expected.py) against a per-base brute
force, the three identities through the existing oracle, and every refusal that needs no GPU.

The identities (all integers, compared exactly):
  * spliced coverage <= plain coverage, cell by cell;
  * plain - spliced == the plain coverage of the gap intervals, taken as reads with their read's flag, mapq and tlen;
  * on reads without N the two are equal.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import spliced_expected as sx
from bamsignals_amd import GRanges, _lib, bamCoverage, bamViews
from bamsignals_amd.synth import synth_reads, tile_ranges

MISSING = os.path.join(GOLDEN, "no_such_file.bam")


@pytest.fixture(scope="module")
def hand():
    return sx.hand_deck()


@pytest.fixture(scope="module")
def rnd():
    return sx.random_deck()


def _plain(cols):
    return dict(cols, end=sx.ends(cols))


def test_hand_deck_holds_what_it_should(hand):
    assert 35 <= len(hand["pos"]) <= 45
    assert hand["pos"][0] == -1
    assert hand["ref_off"][1] == hand["ref_off"][2], "reference 1 stays empty"
    assert np.max(np.diff(hand["cigar_off"])) == sx.LONG_OPS
    # two reads with one pos and different introns
    same = np.flatnonzero((hand["pos"][1:] == hand["pos"][:-1]))
    assert len(same) >= 2


def test_blocks_of_single_reads():
    """the cases of the issue, one by one: (cigar, flag) -> blocks relative to pos"""
    want = {
        ("100M", 0): [(0, 99)],
        ("40M2000N60M", 0): [(0, 39), (2040, 2099)],
        ("10N90M", 0): [(10, 99)],
        ("90M10N", 0): [(0, 89)],
        ("50M5N5N50M", 0): [(0, 49), (60, 109)],
        ("50M5N3I5N50M", 0): [(0, 49), (60, 109)],
        ("10S20M100N30M5H", 0): [(0, 19), (120, 149)],
        ("30M10D30M50N40M", 0): [(0, 69), (120, 159)],
        ("200N", 0): [],
        ("*", 0): [(0, 0)],
        ("50M100N50M", 4): [(0, 0)],
    }
    for (text, flag), blocks in want.items():
        cols = sx.columns([10_000], [(0, 1000, flag, 9, 7, text)])
        b = sx.blocks(cols)
        assert [(int(s) - 1000, int(e) - 1000) for s, e in zip(b["pos"], b["end"])] == blocks, text
        assert np.all(b["flag"] == flag) and np.all(b["mapq"] == 9) and np.all(b["tlen"] == 7)
    g = sx.gaps(sx.columns([10_000], [(0, 1000, 0, 9, 7, "50M5N3I5N50M")]))
    assert list(zip(g["pos"], g["end"])) == [(1050, 1059)], "Ns separated only by I make one gap"


def test_blocks_against_brute_force_on_the_hand_deck(hand):
    b, plain = sx.blocks(hand), _plain(hand)
    assert np.all(np.diff(b["pos"].astype(np.int64) + (np.repeat(np.arange(3), np.diff(b["ref_off"])).astype(np.int64) << 32)) >= 0)
    windows = [(0, 0, 3000), (0, 3900, 4200), (0, 999_990, 1_000_120), (0, 1_999_990, 2_000_140), (0, 2_999_800, 3_000_000),
               (1, 0, 300), (2, 0, 3200), (2, 99_990, 100_100), (2, 169_900, 170_100), (2, 398_900, 400_000)]
    for rid, lo, hi in windows:
        rg = dict(rid=[rid], loc=[lo], len=[hi - lo], strand=[0])
        assert np.array_equal(sx.expected_coverage(b, rg), sx.brute_coverage(hand, rid, lo, hi, True)), (rid, lo, hi)
        assert np.array_equal(sx.expected_coverage(plain, rg), sx.brute_coverage(hand, rid, lo, hi, False)), (rid, lo, hi)


def _identities(cols, width, **flt):
    b, g, plain = sx.blocks(cols), sx.gaps(cols), _plain(cols)
    rg = tile_ranges(cols["ref_len"], width)
    spliced, whole, holes = (sx.expected_coverage(x, rg, **flt) for x in (b, plain, g))
    assert np.all(spliced <= whole)
    assert np.array_equal(whole - spliced, holes)
    return spliced, whole


@pytest.mark.parametrize("flt", [dict(), dict(mapqual=30), dict(filteredF=0x400), dict(requiredF=16), dict(tlen_filter=(0, 200))],
                         ids=["all", "mapq", "filtered", "required", "tlen"])
def test_identities_on_both_decks(hand, rnd, flt):
    for cols in (hand, rnd):
        spliced, whole = _identities(cols, 5000, **flt)
        assert spliced.sum() < whole.sum()


def test_identity_without_n(rnd):
    coff, cig = rnd["cigar_off"], rnd["cigar"]
    keep = np.flatnonzero([not np.any((cig[coff[i]:coff[i + 1]] & 0xF) == 3) for i in range(len(rnd["pos"]))])
    cols = sx.take(rnd, keep)
    assert len(keep) > 500 and len(sx.gaps(cols)["pos"]) == 0
    spliced, whole = _identities(cols, 2048)
    assert np.array_equal(spliced, whole)


def test_random_deck_is_spliced_enough(rnd):
    one, three = sx.n_share(rnd)
    assert len(rnd["pos"]) == 5000 and one >= 0.20 and three >= 0.01, (one, three)
    b = sx.blocks(rnd)
    assert len(b["pos"]) > len(rnd["pos"])


def test_synth_reads_satisfy_the_restatement():
    cols = synth_reads(20000, [1_000_000, 400_000], seed=11)
    one, _ = sx.n_share(cols)
    assert 0.015 <= one <= 0.035, one           # 2 % draw 40M2000N60M
    assert np.array_equal(sx.ends(cols), cols["end"])
    spliced, whole = _identities(cols, 4096)
    b = sx.blocks(cols)
    assert len(b["pos"]) == len(cols["pos"]) + int(round(one * len(cols["pos"])))
    # every intron is 2,000 bases; the ranges tile the references, so what overhangs a reference's end lies in none
    inside = np.minimum(sx.gaps(cols)["end"].astype(np.int64) + 1, cols["ref_len"][np.repeat(np.arange(2), np.diff(sx.gaps(cols)["ref_off"]))]) \
        - sx.gaps(cols)["pos"]
    assert whole.sum() - spliced.sum() == int(np.maximum(inside, 0).sum()) <= 2000 * (len(b["pos"]) - len(cols["pos"]))


# ---- refusals, no GPU -------------------------------------------------------------------------------------------------------
GR = GRanges(["chr1"], [1000], width=[100])


@pytest.mark.parametrize("kwargs, words", [
    (dict(splice=True, paired_end="extend"), 'splice with paired_end="extend"'),
    (dict(splice=True, fragLength=150), "splice with fragLength"),
    (dict(splice=True, fragLength=150, keepDup=1), "splice with fragLength"),
    (dict(splice=True, keepDup=1), "splice with keepDup"),
    (dict(splice=1), "splice must be True or False"),
    (dict(splice="yes"), "splice must be True or False"),
    (dict(splice=None), "splice must be True or False"),
])
def test_bam_coverage_refuses_before_the_file_is_touched(kwargs, words):
    with pytest.raises(ValueError, match=words):
        bamCoverage(MISSING, GR, verbose=False, **kwargs)


@pytest.mark.parametrize("kwargs, words", [
    (dict(signal="ends", splice=True), 'splice with signal="ends"'),
    (dict(signal="coverage", splice=True, paired_end="extend"), 'splice with paired_end="extend"'),
    (dict(signal="coverage", splice=True, fragLength=100), "splice with fragLength"),
    (dict(signal="coverage", splice=0), "splice must be True or False"),
    (dict(signal="ends", splice="no"), "splice must be True or False"),
])
def test_bam_views_refuses_before_the_file_is_touched(kwargs, words):
    with pytest.raises(ValueError, match=words):
        bamViews(MISSING, GR, 1, verbose=False, **kwargs)


def test_reads_spliced_needs_the_cigar_before_any_gpu_call():
    from bamsignals_amd.device import Reads
    with pytest.raises(ValueError, match="spliced reads need cigar_off"):
        Reads(None, [1000], [0, 1], [10], [0], [0], [0], end=[109], spliced=True)


NEW_SYMBOLS = ["bsig_reads_upload_spliced", "bsig_reads_from_bam_spliced", "bsig_reads_from_bam_regions_spliced", "bsig_reads_is_spliced",
               "bsig_coverage_core_spliced", "bsig_coverage_sum_spliced", "bsig_coverage_runs_spliced", "bsig_coverage_views_spliced"]


def test_new_symbols_load():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.bsig_abi_version() == 4
    assert lib.bsig_reads_is_spliced(None) == 0
    abi = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bamsignals_abi.h")).read()
    doc = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in abi and name in doc, name


def _file_call(name, path, binsize=1, ss=0, missing_output=False, lower=1, upper=5):
    """one file-level spliced call on two ranges of the fixture's chromosomes; (code, message)"""
    lib = _lib.load()
    n = 2
    width, start, strand = np.full(n, 100, np.int32), np.full(n, 1000, np.int32), np.ones(n, np.int32)
    codes = np.arange(n, dtype=np.int32) % 2
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.zeros(1, np.int32)
    head = (path.encode(), n, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data, tf.ctypes.data, 0)
    mid = (0, 0, -1, 16385, -1, binsize, ss)
    out, off, wide = np.zeros(4096, np.int32), np.zeros(n + 1, np.int64), np.zeros(4096, np.int64)
    lib.bsig_layout(n, width.ctypes.data, max(binsize, 1), ss, off.ctypes.data)
    handle = C.c_void_p()
    tail = {"bsig_coverage_core_spliced": (None, None) if missing_output else (out.ctypes.data, off.ctypes.data),
            "bsig_coverage_sum_spliced": (None if missing_output else wide.ctypes.data,),
            "bsig_coverage_runs_spliced": (None if missing_output else C.byref(handle),),
            "bsig_coverage_views_spliced": (lower, upper, None if missing_output else C.byref(handle))}[name]
    rc = getattr(lib, name)(*head, *mid, *tail)
    assert handle.value is None, "a refused call hands out no result"
    return rc, lib.bsig_last_error().decode()


FILE_CALLS = ["bsig_coverage_core_spliced", "bsig_coverage_sum_spliced", "bsig_coverage_runs_spliced", "bsig_coverage_views_spliced"]


@pytest.mark.parametrize("name", FILE_CALLS)
def test_file_level_refusals_before_io(name):
    # a bin of 0 bases on a file that does not exist: the parameter is judged first
    rc, msg = _file_call(name, MISSING, binsize=0)
    assert rc == -1 and "binsize" in msg, (rc, msg)
    rc, msg = _file_call(name, MISSING, binsize=65537)
    assert rc == -1, (rc, msg)
    # the output argument, then the file
    rc, msg = _file_call(name, MISSING, missing_output=True)
    assert rc == -1 and "NULL" in msg or "missing" in msg, (rc, msg)
    rc, msg = _file_call(name, MISSING)
    assert rc == -2 and "Fail to open BAM file" in msg, (rc, msg)


def test_views_thresholds_are_judged_before_io():
    rc, msg = _file_call("bsig_coverage_views_spliced", MISSING, lower=5, upper=1)
    assert rc == -1 and "lower (5) is above upper (1)" in msg, (rc, msg)


def test_bam_writer_takes_the_hand_deck(tmp_path):
    """the file-level GPU tests write both decks: the long read goes through the writer's CG tag and comes back whole"""
    from bamsignals_amd.bamio import BamFile, write_columns_as_bam
    hand = sx.hand_deck()
    path = str(tmp_path / "hand.bam")
    write_columns_as_bam(path, ["chr1", "chr2", "chr3"], hand)
    bam = BamFile(path)
    got = bam.decode()
    assert np.array_equal(got["pos"], hand["pos"]) and np.array_equal(got["cigar_off"], hand["cigar_off"])
    assert np.array_equal(got["cigar"], hand["cigar"])
    bam.close()
