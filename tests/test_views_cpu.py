"""CPU: bamViews' host side -- the numpy helper the GPU tests expect with (tests/views_expected.py) against a restatement
that walks cell by cell, the SignalViews container (construction, wider_than, merged, to_granges, to_bed) against views
recomputed from dense rows, and bamViews' argument refusals, which come before the library is touched."""
import numpy as np
import pytest

import views_expected as vx
from bamsignals_amd import GRanges, SignalViews, bamViews

I32 = np.int32
MIN, MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


def walk(v, lower, upper=MAX):
    """the views of one segment, cell by cell"""
    out, cur = [], None
    for p, x in enumerate(np.asarray(v).tolist()):
        if lower <= x <= upper:
            if cur is None:
                cur = [p, 0, 0, x, p]
                out.append(cur)
            cur[1] += 1
            cur[2] += x
            if x > cur[3]:
                cur[3], cur[4] = x, p
        else:
            cur = None
    cols = list(zip(*out)) if out else [[]] * 5
    return tuple(np.asarray(c, dt) for c, dt in zip(cols, vx.DTYPES[1:]))


def test_the_helper_against_a_walk_cell_by_cell():
    rng = np.random.default_rng(5)
    for trial in range(60):
        n = int(rng.integers(0, 400))
        v = rng.integers(-3, 6, n).astype(I32)
        if trial % 7 == 0 and n:
            v[rng.integers(0, n, 5)] = [MIN, MAX, MAX, -1, MIN]
        for lower, upper in ((1, MAX), (2, 3), (MIN, -1), (0, 0), (MIN, MAX), (MAX, MAX), (4, 4)):
            got, want = vx.views_of(v, lower, upper), walk(v, lower, upper)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (trial, lower, upper)
            vx.check_invariants(vx.views_of_segments([v], lower, upper), [v], lower, upper)
    # three neighbours of INT32_MAX: the sum needs 64 bits
    got = vx.views_of(np.asarray([0, MAX, MAX, MAX, 0], I32), 1)
    assert got[2].tolist() == [3 * MAX] and got[4].tolist() == [1]
    # many segments at once are the segments one by one
    length = rng.integers(0, 6, 3000)
    buf = rng.integers(0, 3, int(length.sum())).astype(I32)
    base = np.concatenate([[0], np.cumsum(length)])[:-1]
    vx.same_views(vx.views_of_many(buf, length, 1), vx.views_of_segments(vx.table_segments(buf, base, length, 1), 1))


def test_invariants_catch_wrong_views():
    v = np.asarray([0, 2, 5, 5, 0, 1, 0], I32)
    good = vx.views_of_segments([v], 1)
    vx.check_invariants(good, [v], 1)
    assert [a.tolist() for a in good] == [[0, 2], [1, 5], [3, 1], [12, 1], [5, 1], [2, 5]]
    for k, bad in ((5, [3, 5]), (4, [4, 1]), (3, [11, 1]), (2, [2, 1]), (1, [2, 5])):
        wrong = list(good)
        wrong[k] = np.asarray(bad, good[k].dtype)
        with pytest.raises(AssertionError):
            vx.check_invariants(tuple(wrong), [v], 1)


def dense_rows(rng, n, ss, width=300):
    """rows of a signal with gaps of every small length between the stretches above 0"""
    rows = []
    for _ in range(n * (2 if ss else 1)):
        w = int(rng.integers(0, width))
        v = rng.integers(0, 9, w) * (rng.random(w) < 0.6) * (np.sin(np.arange(w) / 7.0 + rng.random() * 6) > -0.3)
        rows.append(v.astype(I32))
    return rows


def make(rows, lower, upper, ss):
    return SignalViews(*vx.views_of_segments(rows, lower, upper), ss)


def test_construction_and_access():
    rng = np.random.default_rng(6)
    rows = dense_rows(rng, 7, True)
    sv = make(rows, 2, MAX, True)
    assert len(sv) == 7 and sv.ss and sv.nviews == len(sv.start) > 7
    assert sv.counts().shape == (2, 7) and sv.counts().sum() == sv.nviews
    for i in range(7):
        for row in (0, 1):
            want = vx.views_of(rows[2 * i + row], 2)
            assert sv.counts()[row, i] == len(want[0])
            for f, w in zip(SignalViews.FIELDS, want):
                assert np.array_equal(sv[i][row][f], w)
    flat = make(rows, 2, MAX, False)
    assert len(flat) == 14 and flat.counts().shape == (14,) and set(flat[3]) == set(SignalViews.FIELDS)
    assert np.array_equal(flat[-1]["start"], flat[13]["start"])
    for a in (sv.seg_off, sv.start, sv.width, sv.sum, sv.max, sv.summit):
        assert not a.flags.writeable
    with pytest.raises(IndexError):
        flat[14]
    with pytest.raises(TypeError):
        flat["0"]
    empty = SignalViews([0], [], [], [], [], [], False)
    assert len(empty) == 0 and empty.nviews == 0 and len(empty.merged(3)) == 0 and empty.wider_than(2).nviews == 0
    none = SignalViews([0, 0, 0], [], [], [], [], [], True)
    assert len(none) == 1 and none.counts().tolist() == [[0], [0]]


def test_construction_refusals():
    ok = dict(seg_off=[0, 2, 3], start=[1, 5, 0], width=[2, 3, 1], sum=[5, 9, 1], max=[3, 4, 1], summit=[1, 6, 0])
    SignalViews(**ok, ss=False)
    for change in (dict(ss=1), dict(ss=True, seg_off=[0, 2, 3, 3]), dict(seg_off=[1, 2, 3]), dict(seg_off=[0, 3, 2]), dict(seg_off=[0, 2, 4]),
                   dict(seg_off=[]), dict(width=[2, 3]), dict(width=[2, 0, 1]), dict(start=[-1, 5, 0]), dict(summit=[3, 6, 0]),
                   dict(summit=[0, 6, 0]), dict(start=[1, 3, 0]), dict(start=[5, 1, 0], summit=[5, 2, 0])):
        with pytest.raises(ValueError):
            SignalViews(**{**ok, "ss": False, **change})
    # touching is refused inside a segment only
    SignalViews([0, 1, 2], [0, 0], [4, 4], [4, 4], [1, 1], [0, 0], False)


@pytest.mark.parametrize("ss", [False, True])
def test_wider_than(ss):
    rng = np.random.default_rng(7)
    rows = dense_rows(rng, 9, ss)
    sv = make(rows, 1, 6, ss)
    for minwidth in (1, 2, 3, 8):
        got = sv.wider_than(minwidth)
        per = [vx.views_of(r, 1, 6) for r in rows]
        keep = [p[1] >= minwidth for p in per]
        assert np.array_equal(np.diff(got.seg_off), [int(k.sum()) for k in keep])
        for f, k in zip(SignalViews.FIELDS, range(5)):
            want = np.concatenate([p[k][kp] for p, kp in zip(per, keep)])
            assert np.array_equal(getattr(got, f), want), (minwidth, f)
        assert got.ss == ss and len(got) == len(sv)
    assert sv.wider_than(1).nviews == sv.nviews > sv.wider_than(3).nviews > 0


def merged_of(v, lower, upper, maxgap):
    """the joined views of one dense row: the gaps of at most maxgap cells BETWEEN two views closed, the sum over the in-cells"""
    v = np.asarray(v, I32)
    m = (v >= lower) & (v <= upper)
    closed = m.copy()
    at = np.flatnonzero(m)
    for a, b in zip(at[:-1], at[1:]):
        if b - a - 1 <= maxgap:
            closed[a:b] = True
    out = []
    for s, w in zip(*vx.views_of(closed.astype(I32), 1)[:2]):
        inside = np.flatnonzero(m[s:s + w]) + s
        out.append((s, w, int(v[inside].astype(np.int64).sum()), int(v[inside].max()), int(inside[np.argmax(v[inside])])))
    return out


@pytest.mark.parametrize("maxgap", [0, 1, 5])
@pytest.mark.parametrize("ss", [False, True])
def test_merged(ss, maxgap):
    rng = np.random.default_rng(8)
    rows = dense_rows(rng, 9, ss)
    rows.append(np.asarray([3, 0, 3, 0, 0, 7, 0, 0, 0, 0, 0, 7, 9, 0, 0, 0, 0, 0, 0, 9], I32))     # gaps of 1, 2, 5 and 6
    rows.append(np.asarray([4, 4], I32))
    sv = make(rows, 2, 9, ss)
    got = sv.merged(maxgap)
    assert got.ss == ss and len(got) == len(sv)
    n_joined = 0
    for k, r in enumerate(rows):
        want = merged_of(r, 2, 9, maxgap)
        a, b = got.seg_off[k], got.seg_off[k + 1]
        assert [tuple(int(getattr(got, f)[j]) for f in SignalViews.FIELDS) for j in range(a, b)] == want, k
        n_joined += len(vx.views_of(r, 2, 9)[0]) - len(want)
    if maxgap == 0:
        vx.same_views(tuple(getattr(got, f) for f in vx.NAMES), tuple(getattr(sv, f) for f in vx.NAMES))
    else:
        assert n_joined > 0
    with pytest.raises(ValueError):
        sv.merged(-1)


def granges():
    """'+', '-' and '*' ranges; widths that 7 divides and widths with a short last bin"""
    return GRanges(["chr1", "chr2", "chr1", "chr2", "chr1"], [101, 5, 1000, 50, 7], width=[70, 33, 20, 1, 15], strand=["+", "-", "*", "-", "+"])


def per_base(rng, gr):
    return [(rng.integers(0, 7, int(w)) * (rng.random(int(w)) < 0.7)).astype(I32) for w in gr.width]


@pytest.mark.parametrize("binsize", [1, 7])
def test_to_granges_and_to_bed(tmp_path, binsize):
    rng = np.random.default_rng(9)
    gr = granges()
    base = per_base(rng, gr)
    bins = [np.add.reduceat(b, np.arange(0, len(b), binsize)).astype(I32) for b in base]
    lower = 2 if binsize == 1 else 12
    sv = make(bins, lower, MAX, False)
    assert sv.nviews > len(gr)
    path = tmp_path / "v.bed"
    assert sv.to_bed(path, gr, binsize=binsize) == sv.nviews
    lines = open(path).read().splitlines()
    want = []
    for i in range(len(gr)):
        want += vx.lines_per_bin(bins[i], gr.seqnames[i], gr.start[i], gr.width[i], gr.strand[i], i, lower, binsize=binsize)
    assert lines == want
    # read back and expanded: the bases of the in-bins, in ascending genomic order
    for i in range(len(gr)):
        one = SignalViews(np.asarray([0, len(sv[i]["start"])]), *(sv[i][f] for f in SignalViews.FIELDS), False)
        p = tmp_path / f"r{i}.bed"
        one.to_bed(p, gr[i:i + 1], binsize=binsize)
        m = np.repeat((bins[i] >= lower), binsize)[:int(gr.width[i])]
        assert np.array_equal(vx.bed_expand(p, gr.seqnames[i], gr.start[i], gr.width[i]), m[::-1] if gr.strand[i] == "-" else m)
    # the same intervals as genomic ranges: 1-based, with the columns
    out, cols = sv.to_granges(gr, binsize=binsize)
    assert len(out) == sv.nviews == len(cols["sum"])
    for k, line in enumerate(lines):
        f = line.split("\t")
        assert (out.seqnames[k], int(out.start[k]) - 1, int(out.start[k]) - 1 + int(out.width[k]), out.strand[k]) == (f[0], int(f[1]), int(f[2]), f[5])
        assert f[3] == f"range{cols['range'][k]}_{cols['view'][k]}" and int(f[4]) == cols["max"][k] and int(f[6]) == cols["sum"][k]
        assert int(f[7]) == cols["summit"][k] - int(out.start[k])
    # strand-specific: a row has to be chosen
    both = make([b for x in bins for b in (x, x[::-1].copy())], lower, MAX, True)
    with pytest.raises(ValueError):
        both.to_bed(path, gr, binsize=binsize)
    assert both.to_bed(path, gr, binsize=binsize, row="sense") == sv.nviews and open(path).read().splitlines() == lines
    n_anti = both.to_bed(path, gr, binsize=binsize, row=1)
    assert n_anti == int(both.counts()[1].sum())
    with pytest.raises(ValueError):
        sv.to_bed(path, gr, binsize=binsize, row=1)
    with pytest.raises(ValueError):
        sv.to_bed(path, gr[0:2], binsize=binsize)
    with pytest.raises(ValueError):
        sv.to_granges(gr, binsize=0)
    # a view that lies beyond its range's last bin is refused
    beyond = SignalViews([0, 1, 1, 1, 1, 1], [70], [1], [5], [5], [70], False)
    with pytest.raises(ValueError):
        beyond.to_granges(gr, binsize=binsize)


def test_bamviews_refuses_before_any_library_call(monkeypatch):
    from bamsignals_amd import _lib
    gr = granges()

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    for kw in (dict(lower=3, upper=2), dict(lower=1.5), dict(lower=True), dict(lower=1, upper=False), dict(lower="1"),
               dict(lower=2**31), dict(lower=1, upper=-2**31 - 1), dict(lower=np.float64(2.5)),
               dict(lower=1, signal="ends", fragLength=150), dict(lower=1, signal="coverage", shift=10), dict(lower=1, shift=5),
               dict(lower=1, signal="peaks"), dict(lower=1, signal="ends", binsize=0), dict(lower=1, binsize=0),
               dict(lower=1, fragLength=0), dict(lower=1, fragLength=100, paired_end="extend"),
               dict(lower=1, signal="coverage", paired_end="midpoint")):
        with pytest.raises(ValueError):
            bamViews("no_such.bam", gr, verbose=False, **kw)
    with pytest.raises(TypeError):
        bamViews("no_such.bam", "chr1:1-10", 1, verbose=False)
    # whole numbers in other clothes pass the checks and reach the library
    for kw in (dict(lower=2.0), dict(lower=np.int64(2), upper=np.int32(9)), dict(lower=-5, upper=-5), dict(lower=1, signal="ends", shift=20)):
        with pytest.raises(AssertionError, match="touched"):
            bamViews("no_such.bam", gr, verbose=False, **kw)
