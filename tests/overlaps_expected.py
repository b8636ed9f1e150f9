"""The expected side of the bamOverlaps tests (a helper, not a conftest): two independent statements of the definition.
`restated` says it directly in numpy, range by range; `from_oracle` builds the default case (type "any", minoverlap 1,
filteredF -1) from the C oracle's coverage and bamCount alone.  Never the GPU plan."""
import numpy as np

from crosscorr_expected import merge_sorted, oracle_reads  # noqa: F401  (shared column helpers)


def _flat(fwd, rev, strand, ss):
    """counts by the READ's strand -> the plan's layout: n cells, or 2 n as (sense, antisense) pairs; a counted read is
    antisense iff (flag & 16 != 0) != (range strand '-')"""
    fwd, rev = np.asarray(fwd, np.int64), np.asarray(rev, np.int64)
    if not ss:
        return (fwd + rev).astype(np.int32)
    minus = np.asarray(strand) < 0
    out = np.empty(2 * len(fwd), np.int32)
    out[0::2] = np.where(minus, rev, fwd)
    out[1::2] = np.where(minus, fwd, rev)
    return out


def intervals(cols, tlen_filter=(), mapqual=0, requiredF=0, filteredF=-1, tspan=False):
    """per read: does it pass the filter (read_rejected: oracle/bamsignals_oracle.c:91-102), its interval [s, e], its
    strand"""
    pos, end = np.asarray(cols["pos"], np.int64), np.asarray(cols["end"], np.int64)
    flag, mapq = np.asarray(cols["flag"], np.int64), np.asarray(cols["mapq"], np.int64)
    tlen = np.asarray(cols["tlen"], np.int64)
    nf = ~flag
    ok = (mapq >= mapqual) & ((np.int64(requiredF) & nf) == 0) & ((np.int64(filteredF) & nf & 0xFFFFFFFF) != 0)
    if len(tlen_filter) == 2:
        a = np.abs(tlen)
        ok &= (a >= tlen_filter[0]) & (a <= tlen_filter[1])
    neg = (flag & 16) != 0
    s, e = pos.copy(), end.copy()
    if tspan:
        back = neg & (tlen < 0)
        fwd = ~neg & (tlen > 0)
        s[back] = end[back] + tlen[back] + 1
        e[fwd] = pos[fwd] + tlen[fwd] - 1
    return ok, s, e, neg


def restated(cols, rg, within=False, m=1, ss=False, tlen_filter=(), mapqual=0, requiredF=0, filteredF=-1, tspan=False):
    """the definition, range by range: ov = min(e, hi - 1) - max(s, lo) + 1 >= m (within: and s >= lo, e <= hi - 1).
    Only the reads whose pos lies within (longest read + tlen_filter[1]) of the range are looked at: no other can
    reach it (pos is sorted inside a reference)."""
    ok, s, e, neg = intervals(cols, tlen_filter, mapqual, requiredF, filteredF, tspan)
    ref_off = np.asarray(cols["ref_off"], np.int64)
    pos, end = np.asarray(cols["pos"], np.int64), np.asarray(cols["end"], np.int64)
    reach = int((end - pos).max(initial=0)) + 1 + (int(tlen_filter[1]) if tspan else 0)
    n = len(rg["len"])
    fwd, rev = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i, (r, lo, w) in enumerate(zip(rg["rid"], rg["loc"], rg["len"])):
        lo, w = int(lo), int(w)
        if w <= 0:
            continue
        hi = lo + w
        a, b = int(ref_off[r]), int(ref_off[r + 1])
        j0 = a + int(np.searchsorted(pos[a:b], lo - reach, side="left"))
        j1 = a + int(np.searchsorted(pos[a:b], hi + reach, side="right"))
        sl = slice(j0, j1)
        ov = np.minimum(e[sl], hi - 1) - np.maximum(s[sl], lo) + 1
        hit = ok[sl] & (ov >= m)
        if within:
            hit &= (s[sl] >= lo) & (e[sl] <= hi - 1)
        rev[i] = int(np.count_nonzero(hit & neg[sl]))
        fwd[i] = int(np.count_nonzero(hit)) - rev[i]
    return _flat(fwd, rev, rg["strand"], ss)


def from_oracle(orc, rg, ss=False, tlen_filter=(), mapqual=0, requiredF=0, tspan=False):
    """type "any", minoverlap 1, filteredF -1, from the C oracle alone, per strand of the read:
    a forward read overlaps [lo, hi) iff it covers lo (coverage at lo, reverse reads filtered out) or starts behind it
    (bamCount over [lo + 1, hi)); a reverse read iff it covers hi - 1 or ends before it (bamCount over [lo, hi - 1)).
    "extend" moves neither a forward read's start nor a reverse read's end, so bamCount's 5' ends serve there too."""
    from oracle import oracle_c
    rid, loc = np.asarray(rg["rid"], np.int32), np.asarray(rg["loc"], np.int64)
    w = np.asarray(rg["len"], np.int64)
    n = len(w)
    live = w > 0
    one = np.where(live, 1, 0).astype(np.int32)
    rest = np.maximum(w - 1, 0).astype(np.int32)
    strand = np.asarray(rg["strand"], np.int32)

    def ranges(start, length):
        return dict(rid=rid, loc=np.asarray(start, np.int64).astype(np.int32), len=length, strand=np.ones(n, np.int32))

    def cover(start, **kw):
        out, off = oracle_c.coverage_core(orc, ranges(start, one), tlen_filter=tlen_filter, mapqual=mapqual, tspan=tspan, **kw)
        cell = np.zeros(n, np.int64)
        cell[live] = np.asarray(out, np.int64)[np.asarray(off[:-1])[live]]
        return cell

    def count(start, **kw):
        out, _ = oracle_c.pileup_core(orc, ranges(start, rest), tlen_filter=tlen_filter, mapqual=mapqual, binsize=-1, shift=0,
                                      ss=False, **kw)
        return np.asarray(out, np.int64)

    fwd = cover(loc, requiredF=requiredF, filteredF=16) + count(loc + 1, requiredF=requiredF, filteredF=16)
    rev = cover(loc + w - 1, requiredF=requiredF | 16) + count(loc, requiredF=requiredF | 16)
    return _flat(fwd, rev, strand, ss)


def fixture_columns(fx):
    """the fixture BAM's reads (conftest.fixture_reads) under the helpers' column names"""
    return dict(ref_len=fx["ref_len"], ref_off=fx["ref_off"], pos=fx["bam_pos"], end=fx["bam_end"], flag=fx["bam_flag"],
                mapq=fx["bam_mapq"], tlen=fx["bam_tlen"])


def planted(pos, span, reverse=False, tlen=0, flag=None, rid=0, mapq=60):
    """single reads (unsorted columns for merge_sorted): first base pos, `span` bases long"""
    pos = np.atleast_1d(np.asarray(pos, np.int64))
    span = np.broadcast_to(np.asarray(span, np.int64), pos.shape)
    f = (16 if reverse else 0) if flag is None else flag
    return dict(rid=np.full(len(pos), rid, np.int64), pos=pos, end=pos + span - 1, flag=np.full(len(pos), f, np.int64),
                mapq=np.full(len(pos), mapq, np.int64), tlen=np.broadcast_to(np.asarray(tlen, np.int64), pos.shape).copy())


def mixed_ranges(ref_len, seed):
    """the CPU tests' ranges: widths 1 / ~300 / 20,000, whole references, zero widths, duplicates, overhangs on both ends"""
    rng = np.random.default_rng(seed)
    ref_len = np.asarray(ref_len, np.int64)
    rid, loc, w = [], [], []
    for width, k in ((1, 40), (300, 60), (20_000, 12), (0, 4)):
        r = rng.integers(0, len(ref_len), k)
        ww = np.maximum(width + (rng.integers(-40, 41, k) if width == 300 else 0), 0)
        rid.append(r); loc.append(rng.integers(0, ref_len[r] - width)); w.append(np.broadcast_to(ww, (k,)))  # noqa: E702
    for r, L in enumerate(ref_len):                                   # whole references; overhangs on both ends
        rid.append([r, r, r, r]); loc.append([0, -150, L - 100, -7]); w.append([L, 400, 350, L + 50])  # noqa: E702
    rid, loc, w = np.concatenate(rid), np.concatenate(loc), np.concatenate(w)
    dup = rng.integers(0, len(rid), 8)                                # duplicates: each gets its own count
    rid, loc, w = np.concatenate([rid, rid[dup]]), np.concatenate([loc, loc[dup]]), np.concatenate([w, w[dup]])
    strand = np.asarray([1, -1, 0], np.int32)[rng.integers(0, 3, len(rid))]
    return dict(rid=rid.astype(np.int32), loc=loc.astype(np.int32), len=w.astype(np.int32), strand=strand)
