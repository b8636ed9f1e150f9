"""Inputs shared by test_parameter_extremes_gpu.py and test_oracle_extremes.py: reads in clusters on references of
tens of megabases, template lengths of tens of megabases, and ranges placed where reads moved by megabase shifts and
template-length midpoints land (ref: Pileupper::setRead, src/bamsignals.cpp:339-344).

A read's 5' end moves by `shift` (+ |tlen| / 2 with paired.end = "midpoint"): forward reads of a cluster at C land
near C + s, reverse-strand ones near C - s.  Ranges are put there, 2^24 bases to either side (where a position slipped
by the 24-bit range of a multiply would land), at both ends of every reference, and clipped to the reference, so that
some shifted 5' ends fall before its first or past its last base.
"""
import numpy as np

REFS = (48_000_000, 12_000_000, 70_000)
CLUSTER = 150_000
# cluster starts per reference: one at base 0 of each (a window reaching past the reference's start is clipped to its
# first chunk, where every read of the read body's first pass sits), others spread, one at the end of each
CLUSTERS = ((0, 6_000_000, 14_000_000, 24_000_000, 34_000_000, 48_000_000 - CLUSTER),
            (0, 5_500_000, 12_000_000 - CLUSTER),
            (0,))
WIDTHS = (1, 100, 5_000, 32_767, 32_768, 40_000)
TWO31M1 = 2**31 - 1
# template lengths at the filters' edges (tf0, tf1, tf1 +- 1 of the grid), odd and even, and the int32 extreme
SPECIAL_TLEN = (0, 1, 2, 8_000_000, 8_000_001, 8_000_002, 7_999_999, 11_999_999, 12_000_000, 12_000_001,
                16_777_215, 16_777_216, 16_777_217, 19_999_999, 20_000_000, 20_000_001, 29_999_999,
                999_999_999, 1_000_000_000, 1_000_000_001, TWO31M1)

SHIFTS = (0, 4_177_000, -4_177_000, 4_194_305, -4_194_177, 4_300_000, -4_300_000, 5_000_000, -5_000_000,
          2**23, -2**23, 20_000_000, -20_000_000)
# 200: tiles of at most 256 values (k_profile_small) at every width, across the 32,768-base edge of its narrow form
BINSIZES = (-1, 1, 2, 50, 200, 8_192, 8_193, 50_000)
# binsize 50 takes k_profile_small only where the plan's widest range has at most 256 values: ranges of <= 5,000 bases
SMALL_TILE_MAX_W = 5_000
# paired.end = "midpoint" (requiredF = 66: first mate of a proper pair) and filter-only cases: (shift, tlen_filter);
# the last midpoint case has ext = |shift| + tlen_filter[1] = 2^30 exactly
MIDPOINT = ((2_000_000, (0, 12_000_000)), (-2_000_000, (0, 12_000_000)), (0, (0, 20_000_000)),
            (0, (0, 1_000_000_000)), (4_177_000, (0, 2**30 - 4_177_000)))
FILTER_ONLY = ((0, (8_000_000, 8_000_001)), (5_000_000, (8_000_000, 8_000_001)))
COVERAGE_TF = (0, 20_000_000)

# the far case: one reference of 1.2 Gbp, reads at both of its ends, shifts of up to 2^30 bases
FAR_REF = 1_200_000_000
FAR_SHIFTS = (2**30 - 1, -(2**30 - 1), 1_000_000_000, -1_000_000_000)


def _clustered_reads(rng, refs, clusters, n, cluster_w):
    """Columns (sorted by reference, then pos) of about n reads spread evenly over the clusters."""
    n_cl = sum(len(c) for c in clusters)
    per = max(8, n // n_cl)
    pos_l, rid_l = [], []
    for r, (L, starts) in enumerate(zip(refs, clusters)):
        for c0 in starts:
            w = min(cluster_w, L - c0)
            pos_l.append(c0 + rng.integers(0, w, per))
            rid_l.append(np.full(per, r))
    pos = np.concatenate(pos_l).astype(np.int64)
    rid = np.concatenate(rid_l).astype(np.int64)
    m = len(pos)
    # spans: 1-256 for most (the packed class; 1 and 2 included), a tenth longer (classes 1-3)
    span = rng.integers(1, 257, m)
    span[: m // 64] = rng.integers(1, 3, m // 64)
    longer = rng.random(m) < 0.1
    span[longer] = rng.integers(257, 4_000, int(longer.sum()))
    span[rng.random(m) < 0.004] = 70_000
    ref_len = np.asarray(refs, np.int64)
    span = np.minimum(span, ref_len[rid] - 1)
    pos = np.minimum(pos, ref_len[rid] - span)               # every read ends on its reference
    # single-end (0 / 16) and paired-end (99 / 147 / 83 / 163) reads; both strands about equal
    flags = np.asarray([0, 16, 99, 147, 83, 163], np.int64)
    flag = flags[rng.integers(0, len(flags), m)]
    mapq = np.asarray([0, 10, 20, 30, 60], np.int64)[rng.integers(0, 5, m)]
    # |tlen|: most <= 1,000, a real share in [8e6, 3e7], the special values; sign by mate orientation
    a = rng.integers(20, 1_001, m)
    big = rng.random(m) < 0.3
    a[big] = rng.integers(8_000_000, 30_000_001, int(big.sum()))
    sp = rng.random(m) < 0.08
    a[sp] = np.asarray(SPECIAL_TLEN, np.int64)[rng.integers(0, len(SPECIAL_TLEN), int(sp.sum()))]
    sign = np.where((flag == 99) | (flag == 163), 1, -1)
    tlen = np.where(np.isin(flag, (83, 99, 147, 163)), sign * a, 0)
    order = np.lexsort((pos, rid))
    pos, rid, span, flag, mapq, tlen = (x[order] for x in (pos, rid, span, flag, mapq, tlen))
    counts = np.bincount(rid, minlength=len(refs))
    return dict(ref_len=np.asarray(refs, np.int32), ref_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                rid=rid.astype(np.int32), pos=pos.astype(np.int32), end=(pos + span - 1).astype(np.int32),
                flag=flag.astype(np.uint16), mapq=mapq.astype(np.uint8), tlen=tlen.astype(np.int32),
                cigar_off=np.arange(m + 1, dtype=np.int64), cigar=(span.astype(np.uint32) << 4))


def make_reads(n=300_000, seed=5):
    return _clustered_reads(np.random.default_rng(seed), REFS, CLUSTERS, n, CLUSTER)


def make_far_reads(n=200_000, seed=6):
    return _clustered_reads(np.random.default_rng(seed), (FAR_REF,), ((0, FAR_REF - CLUSTER),), n, CLUSTER)


def place_ranges(refs, clusters, shift, hs=(0,), wrap=True, edges=True, per_anchor=2, max_w=None):
    """Ranges where 5' ends of the clusters' reads land under `shift` (and midpoints |tlen| / 2 in `hs`).
    Returns (ranges, rev): rev[i] is the midpoint h of a range placed at C - shift - h, which catches reverse-strand
    reads, and -1 for every other range."""
    widths = WIDTHS if max_w is None else tuple(w for w in WIDTHS if w <= max_w)
    rid, loc, ln, st, rev = [], [], [], [], []
    k = 0

    def add(r, x, rh):
        nonlocal k
        w = widths[k % len(widths)]
        L = refs[r]
        w = min(w, L)
        x = int(min(max(x, 0), L - w))
        rid.append(r); loc.append(x); ln.append(w); st.append((1, -1, 0)[(k // len(widths)) % 3]); rev.append(rh)
        k += 1

    for r, (L, starts) in enumerate(zip(refs, clusters)):
        cw = min(CLUSTER, L)
        for c0 in starts:
            for o in np.linspace(0, cw - min(cw, 40_000), per_anchor).astype(np.int64):
                for h in hs:
                    for sgn in (1, -1):
                        t = c0 + o + sgn * (shift + h)
                        on_ref = -40_000 < t < L
                        if on_ref:
                            add(r, t, h if sgn < 0 else -1)
                            # the reverse-strand reads' own 5' ends lie up to a span past their starts
                            if sgn < 0:
                                add(r, t + 100, h)
                        if wrap:
                            for d in (2**24, -2**24):
                                if 0 <= t + d < L:
                                    add(r, t + d, -1)
        if edges:
            for x in (0, L - 40_000, L - 1):
                add(r, x, -1)
    out = dict(rid=np.asarray(rid, np.int32), loc=np.asarray(loc, np.int32), len=np.asarray(ln, np.int32),
               strand=np.asarray(st, np.int32))
    return out, np.asarray(rev, np.int64)


def rev_hits(out, off, rev, strand, ss, min_h=0):
    """Oracle counts in the ranges placed for reverse-strand reads moved by a midpoint h >= min_h (`rev` of
    place_ranges): (all counts there, the antisense row of those on '+' / '*' ranges, the reverse-strand reads alone:
    antisense on '+' / '*' ranges, sense on '-' ones).  The last two need `ss`, else they are 0."""
    tot, anti, rev_only = 0, 0, 0
    for i in np.flatnonzero(rev >= min_h):
        v = out[off[i]:off[i + 1]].astype(np.int64)
        tot += int(v.sum())
        if ss:
            a = int(v[1::2].sum())
            if strand[i] >= 0:
                anti += a
                rev_only += a
            else:
                rev_only += int(v[0::2].sum())
    return tot, anti, rev_only
