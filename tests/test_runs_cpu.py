"""CPU: the numpy run-length encoder the GPU tests compare against (tests/runs_expected.py) on hand-written cases, the
RunSignals container on arrays built on the host, its bedGraph against lines written out by hand, and the argument rule
of runs=True.  No compute call is made here."""
import numpy as np
import pytest

import runs_expected as rx

I32 = np.int32
MIN, MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


# ---- the numpy encoder -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells,values,lengths", [
    ([], [], []),
    ([7], [7], [1]),
    ([0, 0, 0, 0], [0], [4]),
    ([1, 2, 3], [1, 2, 3], [1, 1, 1]),
    ([0, 0, 1, 1, 1, 0, 2, 2], [0, 1, 0, 2], [2, 3, 1, 2]),
    ([5, 0, 5, 0, 5], [5, 0, 5, 0, 5], [1, 1, 1, 1, 1]),
    ([MIN, MAX, -1, 0, 0, -1, -1, MAX, MIN, MIN], [MIN, MAX, -1, 0, -1, MAX, MIN], [1, 1, 1, 2, 2, 1, 2]),
])
def test_rle_by_hand(cells, values, lengths):
    v, n = rx.rle(np.asarray(cells, I32))
    assert v.dtype == I32 and n.dtype == I32
    assert v.tolist() == values and n.tolist() == lengths


def test_segments_by_hand():
    """a boundary always starts a run (3 | 3 stays two runs), an empty segment has none"""
    segs = [np.asarray(s, I32) for s in ([1, 1, 3], [3, 3], [], [4], [], [4, 4, 0])]
    seg_off, values, lengths = rx.encode_segments(segs)
    assert seg_off.tolist() == [0, 2, 3, 3, 4, 4, 6]
    assert values.tolist() == [1, 3, 3, 4, 4, 0] and lengths.tolist() == [2, 1, 2, 1, 2, 1]
    rx.check_invariants(seg_off, values, lengths, segs)
    assert rx.encode_segments([])[0].tolist() == [0]


def test_table_and_flat_segments_by_hand():
    buf = np.asarray([10, 20, 11, 21, 12, 22, 7, 7, 7], I32)
    segs = rx.table_segments(buf, [0, 1, 6, 9], [3, 3, 3, 0], 2)[:2] + rx.table_segments(buf, [6, 9], [3, 0], 1)
    assert [s.tolist() for s in segs] == [[10, 11, 12], [20, 21, 22], [7, 7, 7], []]
    # bsig_layout's form: range 0 = 3 bins x 2 strands, range 1 empty, range 2 = 3 cells
    flat = rx.flat_segments(buf[:6], [0, 6, 6], True)
    assert [s.tolist() for s in flat] == [[10, 11, 12], [20, 21, 22], [], []]
    assert [s.tolist() for s in rx.flat_segments(buf, [0, 6, 6, 9], False)] == [[10, 20, 11, 21, 12, 22], [], [7, 7, 7]]


def test_the_loop_free_encoder_is_the_same_encoder():
    rng = np.random.default_rng(11)
    length = rng.integers(0, 6, 5000)
    buf = rng.integers(0, 3, int(length.sum())).astype(I32)
    base = np.concatenate([[0], np.cumsum(length)])[:-1]
    segs = rx.table_segments(buf, base, length, 1)
    want = rx.encode_segments(segs)
    rx.same_runs(rx.encode_many(buf, length), want)
    rx.check_invariants(*want, segs)


def test_check_invariants_catches_a_merged_boundary():
    segs = [np.asarray([3, 3], I32), np.asarray([3], I32)]
    with pytest.raises(AssertionError):
        rx.check_invariants(np.asarray([0, 1, 1], np.int64), np.asarray([3], I32), np.asarray([3], I32), segs)
    with pytest.raises(AssertionError):         # a run cut in two inside a segment
        rx.check_invariants(np.asarray([0, 2, 3], np.int64), np.asarray([3, 3, 3], I32), np.asarray([1, 1, 1], I32), segs)


# ---- RunSignals ---------------------------------------------------------------------------------------------------------
def _signals(segs, ss):
    from bamsignals_amd import RunSignals
    return RunSignals(*rx.encode_segments(segs), ss)


def test_runsignals_round_trip():
    rng = np.random.default_rng(5)
    segs = [rng.integers(0, 3, n).astype(I32) for n in (0, 1, 17, 300, 0, 64)]
    sig = _signals(segs, False)
    assert len(sig) == 6 and sig.nruns == len(sig.values) == len(sig.lengths) and not sig.ss
    assert sig.width().tolist() == [0, 1, 17, 300, 0, 64]
    for i, s in enumerate(segs):
        v, n = sig[i]
        assert not v.flags.writeable and not n.flags.writeable
        assert np.array_equal(np.repeat(v, n), s)
        d = sig.decode(i)
        assert d.dtype == I32 and np.array_equal(d, s)
    assert np.array_equal(sig[-1][0], sig[5][0])
    with pytest.raises(IndexError):
        sig[6]
    cs = sig.as_countsignals()
    assert len(cs) == 6 and not cs.ss and all(np.array_equal(a, b) for a, b in zip(cs, segs))
    assert [len(x[0]) for x in sig] == np.diff(sig.seg_off).tolist()
    for a in (sig.seg_off, sig.values, sig.lengths):
        with pytest.raises(ValueError):
            a[:1] = 0


def test_runsignals_round_trip_with_strands():
    rng = np.random.default_rng(6)
    mats = [rng.integers(0, 2, (2, n)).astype(I32) for n in (5, 0, 40)]
    sig = _signals([row for m in mats for row in m], True)
    assert len(sig) == 3 and sig.ss and sig.width().tolist() == [5, 0, 40]
    for i, m in enumerate(mats):
        (sv, sn), (av, an) = sig[i]
        assert np.array_equal(np.repeat(sv, sn), m[0]) and np.array_equal(np.repeat(av, an), m[1])
        d = sig.decode(i)
        assert d.shape == m.shape and d.dtype == I32 and np.array_equal(d, m)
    cs = sig.as_countsignals()
    assert cs.ss and all(np.array_equal(a, b) for a, b in zip(cs, mats))


def test_runsignals_rejects_arrays_that_do_not_fit():
    from bamsignals_amd import RunSignals
    with pytest.raises(ValueError):
        RunSignals([0, 2], [1], [1], False)
    with pytest.raises(ValueError):
        RunSignals([0, 1, 2, 3], [1, 2, 3], [1, 1, 1], True)        # an odd number of segments
    with pytest.raises(ValueError):
        RunSignals([0, 1], [1], [1], 1)


# ---- bedGraph -----------------------------------------------------------------------------------------------------------
def _gr():
    from bamsignals_amd import GRanges
    return GRanges(["chrA", "chrB", "chrA"], [101, 11, 1], width=[10, 10, 4], strand=["+", "-", "*"])


def test_bedgraph_per_base_by_hand(tmp_path):
    #       chrA:101-110 '+'                  chrB:11-20 '-' (range orientation: from base 20 down)   chrA:1-4 '*'
    segs = [[0, 0, 2, 2, 2, 0, 1, 1, 1, 1], [3, 3, 3, 0, 0, 0, 0, 5, 5, 5], [7, 7, 7, 7]]
    sig = _signals([np.asarray(s, I32) for s in segs], False)
    path = tmp_path / "a.bedGraph"
    assert sig.to_bedgraph(path, _gr()) == 5
    by_hand = ["chrA\t102\t105\t2", "chrA\t106\t110\t1",
               "chrB\t10\t13\t5", "chrB\t17\t20\t3",
               "chrA\t0\t4\t7"]
    assert open(path).read().splitlines() == by_hand
    assert sig.to_bedgraph(path, _gr(), zeros=True) == 8
    with_zeros = ["chrA\t100\t102\t0", "chrA\t102\t105\t2", "chrA\t105\t106\t0", "chrA\t106\t110\t1",
                  "chrB\t10\t13\t5", "chrB\t13\t17\t0", "chrB\t17\t20\t3",
                  "chrA\t0\t4\t7"]
    assert open(path).read().splitlines() == with_zeros
    gr = _gr()
    assert rx.bedgraph_lines(segs, gr.seqnames, gr.start, gr.width, gr.strand) == by_hand
    assert rx.bedgraph_lines(segs, gr.seqnames, gr.start, gr.width, gr.strand, zeros=True) == with_zeros
    assert rx.bedgraph_expand(path, "chrB", 11, 10).tolist() == segs[1][::-1]


def test_bedgraph_bins_of_50_with_a_short_last_bin_by_hand(tmp_path):
    from bamsignals_amd import GRanges
    gr = GRanges(["c1", "c1", "c2"], [1001, 1001, 1], width=[120, 120, 100], strand=["+", "-", "*"])
    # 120 bases in bins of 50: bins of 50, 50 and 20 bases; the '-' range's short bin is at its genomic START
    segs = [[4, 4, 9], [4, 4, 9], [0, 6]]
    sig = _signals([np.asarray(s, I32) for s in segs], False)
    path = tmp_path / "b.bedGraph"
    assert sig.to_bedgraph(path, gr, binsize=50) == 5
    by_hand = ["c1\t1000\t1100\t4", "c1\t1100\t1120\t9",
               "c1\t1000\t1020\t9", "c1\t1020\t1120\t4",
               "c2\t50\t100\t6"]
    assert open(path).read().splitlines() == by_hand
    assert rx.bedgraph_lines(segs, gr.seqnames, gr.start, gr.width, gr.strand, binsize=50) == by_hand
    with pytest.raises(ValueError):
        sig.to_bedgraph(path, gr, binsize=1)              # 3 cells are not 120 bases


def test_bedgraph_with_strands_needs_a_row(tmp_path):
    from bamsignals_amd import GRanges
    gr = GRanges(["c1"], [5], width=[3], strand=["-"])
    sig = _signals([np.asarray([1, 1, 2], I32), np.asarray([0, 8, 8], I32)], True)
    path = tmp_path / "c.bedGraph"
    with pytest.raises(ValueError):
        sig.to_bedgraph(path, gr)
    sig.to_bedgraph(path, gr, row=0)
    assert open(path).read().splitlines() == ["c1\t4\t5\t2", "c1\t5\t7\t1"]
    sig.to_bedgraph(path, gr, row="antisense")
    assert open(path).read().splitlines() == ["c1\t4\t6\t8"]
    with pytest.raises(ValueError):
        sig.to_bedgraph(path, gr, row=2)
    with pytest.raises(ValueError):
        _signals([np.asarray([1], I32)], False).to_bedgraph(path, gr[0:1], row=1)


# ---- the argument rule ----------------------------------------------------------------------------------------------------
def test_runs_with_aggregate_raises_before_any_library_call(monkeypatch):
    import inspect

    from bamsignals_amd import GRanges, _lib, bamCount, bamCoverage, bamProfile, wrappers

    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(wrappers, "_check_gr", no_library)
    gr = GRanges(["c1"], [1], width=[10])
    for call in (bamCoverage, bamProfile):
        with pytest.raises(ValueError, match="runs=True and aggregate=True"):
            call("/nonexistent.bam", gr, runs=True, aggregate=True, verbose=False)
        p = inspect.signature(call).parameters["runs"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert "runs" not in inspect.signature(bamCount).parameters


def test_file_level_checks_its_parameters_first():
    """bamCount's layout and bad parameters are refused before the BAM is opened: a file that does not exist is not missed"""
    import ctypes as C
    from bamsignals_amd import _lib
    lib = _lib.load()
    from bamsignals_amd import GRanges
    gr = GRanges(["chr1", "chr2"], [10, 20], width=[100, 50], strand=["+", "-"])
    levels, codes, start, width, strand = gr.flatten()
    names = (C.c_char_p * len(levels))(*[s.encode() for s in levels])
    head = (b"/nonexistent/file.bam", len(gr), codes.ctypes.data, len(levels), names, start.ctypes.data, width.ctypes.data,
            strand.ctypes.data, None, 0)
    h = C.c_void_p()
    for binsize in (-1, 0):
        assert lib.bsig_pileup_runs(*head, 0, binsize, 0, 0, 0, -1, 0, 16385, 0, C.byref(h)) == -1 and not h.value
    assert lib.bsig_coverage_runs(*head, 0, 0, -1, 0, 16385, 0, 70_000, 0, C.byref(h)) == -1 and not h.value
    assert lib.bsig_coverage_runs(*head, 0, 0, -1, 0, 16385, 0, 1, 0, C.byref(h)) == -2             # BSIG_ERR_IO: now it is opened
