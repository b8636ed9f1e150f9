"""The expected side of the views tests (a helper, not a conftest): the views of one segment by plain numpy, the segments
of a buffer / of a flat per-range result (tests/runs_expected.py), and the invariants any set of views has to meet.
Never the library's own views."""
import numpy as np

from runs_expected import encode_segments, flat_segments, table_segments  # noqa: F401  (the segments are the runs tests')

NAMES = ("seg_off", "start", "width", "sum", "max", "summit")
DTYPES = (np.int64, np.int32, np.int32, np.int64, np.int32, np.int32)
MAX = np.iinfo(np.int32).max


def views_of(v, lower, upper=MAX):
    """(start, width, sum, max, summit) of one segment: the edges of the in-mask, np.add.reduceat in int64 and the first
    argmax per view"""
    v = np.asarray(v, np.int32)
    m = (v >= lower) & (v <= upper)
    edge = np.diff(np.concatenate([[False], m, [False]]).astype(np.int8))
    start, end = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    if len(start) == 0:
        return tuple(np.zeros(0, dt) for dt in DTYPES[1:])
    cuts = np.stack([start, end], axis=1).reshape(-1)               # reduceat over [start, end) and the gaps behind them
    total = np.add.reduceat(np.concatenate([v.astype(np.int64), [0]]), cuts)[0::2]
    vmax = np.maximum.reduceat(np.concatenate([v, [v[0]]]), cuts)[0::2]
    # the first argmax per view: the smallest index among the view's cells that hold its max
    view = np.cumsum(edge[:-1] == 1) - 1
    holds = m & (v == vmax[np.maximum(view, 0)])
    summit = np.minimum.reduceat(np.concatenate([np.where(holds, np.arange(len(v)), len(v)), [len(v)]]), cuts)[0::2]
    return (start.astype(np.int32), (end - start).astype(np.int32), total.astype(np.int64), vmax.astype(np.int32),
            summit.astype(np.int32))


def views_of_segments(segs, lower, upper=MAX):
    """(seg_off, start, width, sum, max, summit) of a list of segments, each by itself"""
    per = [views_of(s, lower, upper) for s in segs]
    seg_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in per])]).astype(np.int64)
    cols = [np.concatenate([p[k] for p in per]).astype(dt) if per else np.zeros(0, dt) for k, dt in enumerate(DTYPES[1:])]
    return (seg_off, *cols)


def views_of_many(buf, length, lower, upper=MAX):
    """views_of_segments for MANY segments that lie behind each other in `buf` (stride 1), without a Python loop: an
    out-cell is put behind every segment, the whole is one segment for views_of, and the views go back to their segments"""
    buf, length = np.asarray(buf, np.int32), np.asarray(length, np.int64)
    assert lower > np.iinfo(np.int32).min and length.sum() == len(buf)
    cell0 = np.concatenate([[0], np.cumsum(length)])
    seg = np.repeat(np.arange(len(length)), length)
    padded = np.full(len(buf) + len(length), lower - 1, np.int32)
    padded[np.arange(len(buf)) + seg] = buf
    start, width, total, vmax, summit = views_of(padded, lower, upper)
    first = cell0[:-1] + np.arange(len(length))                     # where a segment begins in the padded buffer
    owner = np.searchsorted(first, start, side="right") - 1
    seg_off = np.searchsorted(owner, np.arange(len(length) + 1), side="left").astype(np.int64)
    return (seg_off, (start - first[owner]).astype(np.int32), width, total, vmax, (summit - first[owner]).astype(np.int32))


def same_views(got, want):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def check_invariants(got, segs, lower, upper=MAX):
    """what the definition asks of any views of `segs`, without reference to another encoder"""
    seg_off, start, width, total, vmax, summit = got
    for a, dt in zip(got, DTYPES):
        assert a.dtype == dt
    assert len(seg_off) == len(segs) + 1 and seg_off[0] == 0 and np.all(np.diff(seg_off) >= 0)
    assert seg_off[-1] == len(start) == len(width) == len(total) == len(vmax) == len(summit)
    assert np.all(width >= 1)
    for k, s in enumerate(segs):
        s = np.asarray(s, np.int32)
        a, b = int(seg_off[k]), int(seg_off[k + 1])
        st, wd = start[a:b].astype(np.int64), width[a:b].astype(np.int64)
        assert np.all(st >= 0) and np.all(st + wd <= len(s))
        assert np.all(st[1:] > (st + wd)[:-1])                      # ascending, and a cell between two views
        m = (s >= lower) & (s <= upper)
        covered = np.zeros(len(s) + 1, np.int64)
        np.add.at(covered, st, 1)
        np.add.at(covered, st + wd, -1)
        assert np.array_equal(np.cumsum(covered)[:-1].astype(bool), m)   # the cells of the views are the in-cells, all of them
        # sum, max and summit from the cells: the views' cells are the in-cells in ascending order
        csum = np.concatenate([[0], np.cumsum(s.astype(np.int64))])
        assert np.array_equal(total[a:b], csum[st + wd] - csum[st])
        pos, view = np.flatnonzero(m), np.repeat(np.arange(b - a), wd)
        mx, at = vmax[a:b], summit[a:b].astype(np.int64)
        assert np.all((at >= st) & (at < st + wd)) and np.array_equal(s[at], mx)
        assert np.all(s[pos] <= mx[view]) and np.all((s[pos] < mx[view]) | (pos >= at[view]))


def lines_per_bin(signal, chrom, start, width, strand, i, lower, upper=MAX, binsize=1):
    """The BED lines of ONE range's signal (a vector of bins in range orientation), said per BIN: every bin is an interval
    in 0-based half-open genomic coordinates (a '-' range mirrored back, the last bin cut at the range's end); in
    ascending order the in-bins that touch are joined."""
    loc, w = int(start) - 1, int(width)
    ivs = []
    for j, x in enumerate(np.asarray(signal).tolist()):
        lo, hi = j * binsize, min((j + 1) * binsize, w)
        ivs.append((loc + w - hi, loc + w - lo, x, j) if strand == "-" else (loc + lo, loc + hi, x, j))
    ivs.sort()
    views, cur = [], None
    for a, b, x, j in ivs:
        if lower <= x <= upper:
            if cur is None:
                cur = dict(a=a, b=b, sum=0, max=None, at=None, cells=[])
                views.append(cur)
            cur["b"] = b
            cur["sum"] += x
            cur["cells"].append(j)
            # the summit is the first cell in RANGE orientation that holds the max
            if cur["max"] is None or x > cur["max"] or (x == cur["max"] and j < cur["j"]):
                cur["max"], cur["at"], cur["j"] = x, a, j
        else:
            cur = None
    # the view's index inside its segment counts in range orientation
    order = sorted(range(len(views)), key=lambda k: min(views[k]["cells"]))
    index = {k: n for n, k in enumerate(order)}
    return [f"{chrom}\t{v['a']}\t{v['b']}\trange{i}_{index[k]}\t{v['max']}\t{strand}\t{v['sum']}\t{v['at'] - v['a']}" for k, v in enumerate(views)]


def bed_expand(path, chrom, start, width):
    """a BED file of views read back as the per-BASE in-mask of the genomic interval [start - 1, start - 1 + width) of
    `chrom`, ascending; a base two lines cover is an error"""
    seen = np.zeros(int(width), bool)
    loc = int(start) - 1
    for line in open(path).read().splitlines():
        f = line.split("\t")
        a, b = int(f[1]) - loc, int(f[2]) - loc
        if f[0] != chrom or b <= 0 or a >= width:
            continue
        assert 0 <= a < b <= width and not seen[a:b].any(), line
        seen[a:b] = True
    return seen
