"""The expected side of the run-length tests (a helper, not a conftest): a plain numpy run-length encoder per segment,
the segments of a flat per-range result (the C oracle's, or a golden vector), and the bedGraph said again per bin.
Never the library's own per-range result, never its encoder."""
import numpy as np


def rle(v):
    """(values, lengths) of one segment: its maximal stretches of equal consecutive cells"""
    v = np.asarray(v, np.int32)
    if len(v) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    starts = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    return v[starts], np.diff(np.concatenate([starts, [len(v)]])).astype(np.int32)


def encode_segments(segs):
    """(seg_off int64, values int32, lengths int32) of a list of segments, each encoded by itself"""
    enc = [rle(s) for s in segs]
    seg_off = np.concatenate([[0], np.cumsum([len(v) for v, _ in enc])]).astype(np.int64)
    values = np.concatenate([v for v, _ in enc]) if enc else np.zeros(0, np.int32)
    lengths = np.concatenate([n for _, n in enc]) if enc else np.zeros(0, np.int32)
    return seg_off, values.astype(np.int32), lengths.astype(np.int32)


def table_segments(buf, base, length, stride):
    """the segments of a buffer by a table: segment k = buf[base[k] + p * stride], p < length[k]"""
    buf = np.asarray(buf, np.int32)
    return [buf[int(b):int(b) + int(n) * stride:stride] for b, n in zip(base, length)]


def encode_many(buf, length):
    """encode_segments for MANY segments that lie behind each other in `buf` (stride 1), without a Python loop: a cell
    starts a run iff it is first in its segment or differs from the cell before it"""
    buf = np.asarray(buf, np.int32)
    length = np.asarray(length, np.int64)
    cell0 = np.concatenate([[0], np.cumsum(length)])
    assert cell0[-1] == len(buf)
    start = np.ones(len(buf), bool)
    start[1:] = buf[1:] != buf[:-1]
    start[cell0[:-1][length > 0]] = True
    at = np.flatnonzero(start)
    seg_off = np.searchsorted(at, cell0, side="left").astype(np.int64)
    return seg_off, buf[at], np.diff(np.concatenate([at, [len(buf)]])).astype(np.int32)


def flat_segments(flat, off, ss):
    """the segments of a flat per-range result in bsig_layout's form: range i's cells flat[off[i]:off[i + 1]], with ss
    the cells 2 * bin + antisense -> segment 2 * i (sense) and 2 * i + 1 (antisense)"""
    flat = np.asarray(flat)
    segs = []
    for a, b in zip(off[:-1], off[1:]):
        cells = flat[int(a):int(b)]
        segs += [cells[0::2], cells[1::2]] if ss else [cells]
    return segs


def encode_flat(flat, off, ss):
    return encode_segments(flat_segments(flat, off, ss))


def check_invariants(seg_off, values, lengths, segs):
    """what the issue asks of any encoding of `segs`, without reference to another encoder"""
    assert seg_off.dtype == np.int64 and values.dtype == np.int32 and lengths.dtype == np.int32
    assert len(seg_off) == len(segs) + 1 and seg_off[0] == 0 and seg_off[-1] == len(values) == len(lengths)
    assert np.all(lengths >= 1)
    same = np.flatnonzero(values[1:] == values[:-1]) + 1          # equal neighbours: only across a segment boundary
    assert np.all(np.isin(same, seg_off))
    ends = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)])[seg_off]
    assert np.array_equal(np.diff(ends), [len(s) for s in segs])
    flat = np.concatenate([np.asarray(s, np.int32) for s in segs]) if segs else np.zeros(0, np.int32)
    assert np.array_equal(np.repeat(values, lengths), flat)


def same_runs(got, want):
    for g, w, name in zip(got, want, ("seg_off", "values", "lengths")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def bedgraph_lines(signals, chrom, start, width, strand, binsize=1, zeros=False):
    """The bedGraph of per-range signals (one vector of bins per range, in range orientation), said per BIN: every bin
    is an interval in 0-based half-open genomic coordinates (a '-' range mirrored back, the last bin cut at the range's
    end); in ascending order, neighbours of one value are merged; zeros are dropped unless asked for."""
    lines = []
    for sig, c, s, w, st in zip(signals, chrom, start, width, strand):
        loc, w = int(s) - 1, int(w)
        ivs = []
        for j, x in enumerate(np.asarray(sig).tolist()):
            lo, hi = j * binsize, min((j + 1) * binsize, w)
            ivs.append((loc + w - hi, loc + w - lo, x) if st == "-" else (loc + lo, loc + hi, x))
        ivs.sort()
        merged = []
        for a, b, x in ivs:
            if merged and merged[-1][2] == x and merged[-1][1] == a:
                merged[-1][1] = b
            else:
                merged.append([a, b, x])
        lines += [f"{c}\t{a}\t{b}\t{x}" for a, b, x in merged if zeros or x != 0]
    return lines


def bedgraph_expand(path, chrom, start, width):
    """a bedGraph file read back as the per-BASE vector of the genomic interval [start - 1, start - 1 + width) of
    `chrom`, ascending; bases no line covers are 0, a base two lines cover is an error"""
    out = np.zeros(int(width), np.int64)
    seen = np.zeros(int(width), bool)
    loc = int(start) - 1
    for line in open(path).read().splitlines():
        c, a, b, x = line.split("\t")
        a, b = int(a) - loc, int(b) - loc
        if c != chrom or b <= 0 or a >= width:
            continue
        assert 0 <= a < b <= width and not seen[a:b].any(), line
        out[a:b] = int(x)
        seen[a:b] = True
    return out
