"""The input of tests/test_kernel_forms_gpu.py, and what the C oracle says about it (tests/test_forms_deck_cpu.py checks
the deck's own claims without a GPU).  Everything is exact int32 / int64.

Reads (coordinate-sorted columns, seeded):
  * three bulk references of 70,000, 65,536 and 65,537 bp with 20,000 reads each: spans 1 .. 70,000 with the class
    borders 1, 255, 256, 257, 4,095, 4,096, 4,097, 65,535, 65,536 and 65,537 among them, mapq 0 .. 255, the flags 0x4
    and 0x400, paired flags with a template length, and a share of rare (flag, mapq) pairs that the packed class's table
    has no room for;
  * 48 "short" island references of 4,096 bp that hold exactly m reads each, all of them starting in [1024, 3072), of
    span 1 .. 256, flag 0 or 16 and one mapq -- packed in the default layout, class 0 with BAMSIGNALS_PACK=0 -- for m in
    ISLAND_COUNTS: a reference is its own run of 64-kbp units, so the window of a range over [1024, 3072) holds exactly
    its m reads (for_each_read's nj), and the window starts at the number of reads of that class in front of it;
  * 24 "long" islands with the counts up to 769: m reads of span 257 .. 4,096 (class 1) and m of span 4,097 .. 9,000
    (class 2) each;
  * behind them, for the reductions (tests/test_reduction_forms_gpu.py) and the 16-bit columns of span classes 0 and 1,
    two groups of 33 islands with the counts up to 2,049 (NT - 1, NT, NT + 1 and 8 NT - 1, 8 NT, 8 NT + 1 for NT = 64,
    128 and 256), each in a seeded order of its own: "class-0" islands of m reads of span 1 .. 256 whose flags carry bit
    12 (0x1000 / 0x1010; a seeded half of them first of a proper pair, 0x1063 / 0x1053, with a template length of
    +-50 .. 600) -- a flag of more than 12 bits has no code, so these stay in class 0 in the default layout too and a
    range over [1024, 3072) has a class-0 window of exactly m reads --, and "paired" islands of m reads with the flags
    99 / 83 and a template length, which the default layout packs.

Ranges: every width of WIDTHS 16 times on the bulk references in a seeded order (all strands, one at base 0, one that
ends on a last base, some hanging over both ends, duplicates, every width at all four values of out_off & 3), then one
range [1024, 3072) per island.  `cut` drops the last few bulk ranges so that the tiles number a chosen residue modulo 8.  SUM_RANGES
are ranges of one width for the sums over ranges."""
import functools

import numpy as np

ISLAND_KS = (64, 128, 256, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 10240)
ISLAND_COUNTS = tuple(sorted({0, 1, 2, 3, 4, 5, 7, 8, 9} | {k + d for k in ISLAND_KS for d in (-1, 0, 1)}))
LONG_COUNTS = tuple(m for m in ISLAND_COUNTS if m <= 769)
C0_COUNTS = tuple(m for m in ISLAND_COUNTS if m <= 2049)     # the class-0 and the paired islands (33, 19,047 reads a group)
BULK_REFS = (70_000, 65_536, 65_537)
BULK_READS = 20_000                      # per bulk reference
ISLAND_LEN, ISLAND_LO, ISLAND_HI = 4096, 1024, 3072
ISLAND_MAPQ = 30
TILES = (64, 256, 2048)                  # the tile sizes (cells) the matrix runs the per-base forms at
WIDTHS = tuple(sorted(set(range(10)) | {63, 64, 65, 255, 256, 257} | {w for t in TILES for w in (t - 1, t, t + 1, 2 * t + 3)}))
COPIES = 16
SPAN_EDGES = (1, 255, 256, 257, 4095, 4096, 4097, 65_535, 65_536, 65_537)
SUM_WIDTH = 2048

# name -> (oracle entry, its arguments): every set of call parameters the matrix compares
PARAM_SETS = {
    "half_ss0": ("pileup", dict(binsize=1, shift=0, ss=False)),
    "half_ss1": ("pileup", dict(binsize=1, shift=0, ss=True)),
    "word_ss0": ("pileup", dict(binsize=1, shift=75, mapqual=10, ss=False)),
    "word_ss1": ("pileup", dict(binsize=1, shift=75, mapqual=10, ss=True)),
    "small_ss0": ("pileup", dict(binsize=7, shift=0, ss=False)),
    "small_ss1": ("pileup", dict(binsize=7, shift=0, ss=True)),
    "count": ("pileup", dict(binsize=-1, shift=0, ss=True)),
    "cover": ("coverage", dict(binsize=1, ss=False)),
    "bins2_ss0": ("coverage", dict(binsize=2, ss=False)),
    "bins2_ss1": ("coverage", dict(binsize=2, ss=True)),
    "bins274_ss1": ("coverage", dict(binsize=274, ss=True)),
}
SUM_SETS = {
    "sum_half_ss0": ("pileup", dict(binsize=1, shift=0, ss=False)),
    "sum_half_ss1": ("pileup", dict(binsize=1, shift=0, ss=True)),
    "sum_word_ss0": ("pileup", dict(binsize=1, shift=75, mapqual=10, ss=False)),
    "sum_word_ss1": ("pileup", dict(binsize=1, shift=75, mapqual=10, ss=True)),
    "sum_cover": ("coverage", dict(binsize=1, ss=False)),
    "sum_cover_ss": ("coverage", dict(binsize=1, ss=True)),
}


# ---------------------------------------------------------------------------------------------------------------
# reads
# ---------------------------------------------------------------------------------------------------------------
def _bulk(rng, ref_len):
    n = BULK_READS
    pos = rng.integers(0, ref_len, n)
    u = rng.random(n)
    span = rng.integers(1, 257, n)
    c1, c2, c3 = (u >= 0.90) & (u < 0.97), (u >= 0.97) & (u < 0.995), u >= 0.995
    span[c1] = rng.integers(257, 4097, int(c1.sum()))
    span[c2] = rng.integers(4097, 65_537, int(c2.sum()))
    span[c3] = rng.integers(65_537, 70_001, int(c3.sum()))
    edge = rng.random(n) < 0.05                                  # the borders of the span classes, many times each
    span[edge] = np.asarray(SPAN_EDGES)[rng.integers(0, len(SPAN_EDGES), int(edge.sum()))]
    flags = np.asarray([0, 16, 0, 16, 4, 20, 0x400, 0x410, 99, 147, 83, 163])
    flag = flags[rng.integers(0, len(flags), n)]
    mapq = np.asarray([0, 10, 30, 60, 255])[rng.integers(0, 5, n)]
    rare = rng.random(n) < 0.03                                  # pairs the 512-entry table has no room for
    flag[rare] = rng.integers(0, 4096, int(rare.sum()))
    mapq[rare] = rng.integers(1, 255, int(rare.sum()))
    paired = (flag & 1) != 0
    tlen = np.where(paired, rng.integers(50, 601, n) * np.where((flag & 16) != 0, -1, 1), 0)
    return pos, span, flag, mapq, tlen


def _island(rng, m, lo_span, hi_span):
    pos = rng.integers(ISLAND_LO, ISLAND_HI, m)
    span = rng.integers(lo_span, hi_span + 1, m)
    if m >= 3 and lo_span == 1:
        span[:3] = (1, 255, 256)
    flag = np.where(rng.random(m) < 0.5, 16, 0)
    return pos, span, flag, np.full(m, ISLAND_MAPQ), np.zeros(m, np.int64)


def _tlen(rng, flag):
    """a template length of +-50 .. 600, negative for a reverse read"""
    return rng.integers(50, 601, len(flag)) * np.where((np.asarray(flag) & 16) != 0, -1, 1)


def _island_c0(rng, m):
    """m reads that no layout packs (bit 12 of the flag), a seeded half of them first of a proper pair -- the island's
    first read among them, a forward one: its 5' end lies in the island's range whatever its span"""
    pos, span, flag, mapq, tlen = _island(rng, m, 1, 256)
    first = rng.permutation(m) < (m + 1) // 2
    if m:
        # read 0 becomes a forward first-of-pair read; if it was none, the earliest one gives up its place: half stay
        if not first[0]:
            first[np.flatnonzero(first)[0]] = False
            first[0] = True
        flag[0] = 0
    flag = np.where(first, np.where(flag != 0, 0x1053, 0x1063), 0x1000 | flag)
    return pos, span, flag, mapq, np.where(first, _tlen(rng, flag), 0)


def _island_paired(rng, m):
    """m first-of-pair reads (99 forward, 83 reverse; the island's first read forward) with a template length: frequent
    pairs, packed by default"""
    pos, span, flag, mapq, _ = _island(rng, m, 1, 256)
    flag[:1] = 0
    flag = np.where(flag != 0, 83, 99)
    return pos, span, flag, mapq, _tlen(rng, flag)


def _permuted(rng, counts):
    """a seeded order of the islands' counts in which the reads in front of an island -- its window's start, up to the
    bulk references' share -- take every residue modulo 8"""
    for _ in range(100):
        m = rng.permutation(np.asarray(counts))
        start = np.concatenate([[0], np.cumsum(m[:-1])])
        if set((start[m > 0] % 8).tolist()) == set(range(8)):
            return m
    raise AssertionError("no order of the islands with every window start modulo 8")


@functools.lru_cache(maxsize=None)
def reads(placement=None):
    """dict(ref_len, ref_off, pos, end, flag, mapq, tlen, short_refs, long_refs, c0_refs, pair_refs, short_m, long_m, c0_m,
    pair_m): the columns, and the islands' reference ids with their read counts (in reference order, a seeded
    permutation of the counts).  placement (a far_deck.Placement; here and in every function below): the deck moved
    to far coordinates -- the same code on the placed columns and ranges, cached per placement."""
    if placement is not None:
        import far_deck
        return far_deck.place_columns(reads(), placement)
    rng = np.random.default_rng(20_250)
    parts, ref_len = [], list(BULK_REFS)
    for L in BULK_REFS:
        parts.append(_bulk(rng, L))
    short_m, long_m = _permuted(rng, ISLAND_COUNTS), _permuted(rng, LONG_COUNTS)
    for m in short_m:
        parts.append(_island(rng, int(m), 1, 256))
        ref_len.append(ISLAND_LEN)
    for m in long_m:
        a, b = _island(rng, int(m), 257, 4096), _island(rng, int(m), 4097, 9000)
        parts.append(tuple(np.concatenate([x, y]) for x, y in zip(a, b)))
        ref_len.append(ISLAND_LEN)
    # (the later groups draw from generators of their own: the reads above are what they were before these came)
    rng0, rng4 = np.random.default_rng(20_251), np.random.default_rng(20_252)
    c0_m, pair_m = _permuted(rng0, C0_COUNTS), _permuted(rng4, C0_COUNTS)
    for m in c0_m:
        parts.append(_island_c0(rng0, int(m)))
        ref_len.append(ISLAND_LEN)
    for m in pair_m:
        parts.append(_island_paired(rng4, int(m)))
        ref_len.append(ISLAND_LEN)
    cols = {k: [] for k in ("pos", "span", "flag", "mapq", "tlen")}
    counts = []
    for pos, span, flag, mapq, tlen in parts:
        order = np.argsort(pos, kind="stable")
        for k, v in zip(("pos", "span", "flag", "mapq", "tlen"), (pos, span, flag, mapq, tlen)):
            cols[k].append(np.asarray(v, np.int64)[order])
        counts.append(len(pos))
    pos, span = np.concatenate(cols["pos"]), np.concatenate(cols["span"])
    nb = len(BULK_REFS)
    first = np.cumsum([nb, len(short_m), len(long_m), len(c0_m), len(pair_m)])
    return dict(ref_len=np.asarray(ref_len, np.int32), ref_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                pos=pos.astype(np.int32), end=(pos + span - 1).astype(np.int32),
                flag=np.concatenate(cols["flag"]).astype(np.uint16), mapq=np.concatenate(cols["mapq"]).astype(np.uint8),
                tlen=np.concatenate(cols["tlen"]).astype(np.int32),
                short_refs=np.arange(first[0], first[1]), long_refs=np.arange(first[1], first[2]),
                c0_refs=np.arange(first[2], first[3]), pair_refs=np.arange(first[3], first[4]),
                short_m=short_m, long_m=long_m, c0_m=c0_m, pair_m=pair_m)


def read_classes(packed):
    """The class the resident layout gives every read (csrc/bsig_types.h): 0 .. 3 by span (<= 256, <= 4,096, <= 65,536,
    longer), 4 = packed (the default layout; none with BAMSIGNALS_PACK=0)."""
    from conftest import expected_packed
    c = reads()
    span = c["end"].astype(np.int64) - c["pos"] + 1
    cls = np.where(span <= 256, 0, np.where(span <= 4096, 1, np.where(span <= 65_536, 2, 3)))
    if packed:
        cls[expected_packed(c["pos"], c["end"], c["flag"], c["mapq"], c["ref_off"], c["ref_len"])[0]] = 4
    return cls


def island_windows(packed, cls_id, refs):
    """(start, count) of class `cls_id`'s window over each of the island references `refs`: the reads of the class in
    front of the reference, and on it."""
    c = reads()
    is_c = read_classes(packed) == cls_id
    before = np.concatenate([[0], np.cumsum(is_c)])
    lo, hi = c["ref_off"][refs], c["ref_off"][np.asarray(refs) + 1]
    return before[lo], before[hi] - before[lo]


def oracle_reads(mask=None, placement=None):
    from oracle import oracle_c
    c = _reads(placement)
    if mask is None:
        return oracle_c.OracleReads(c["ref_off"], c["pos"], c["end"], c["flag"], c["mapq"], c["tlen"])
    rid = np.repeat(np.arange(len(c["ref_len"])), np.diff(c["ref_off"]))
    off = np.concatenate([[0], np.cumsum(np.bincount(rid[mask], minlength=len(c["ref_len"])))]).astype(np.int64)
    return oracle_c.OracleReads(off, c["pos"][mask], c["end"][mask], c["flag"][mask], c["mapq"][mask], c["tlen"][mask])


def _reads(placement):
    return reads() if placement is None else reads(placement)       # (one cache key for the deck where it is)


def _ranges(placement):
    return ranges() if placement is None else ranges(placement)


def _sum_ranges(placement):
    return sum_ranges() if placement is None else sum_ranges(placement)


def named_placement(name):
    """far_deck's placement `name` of this deck: `top` is computed from its reads and both range tables"""
    import far_deck
    return far_deck.placement(name, reads(), ranges(), sum_ranges())


# ---------------------------------------------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------------------------------------------
def island_refs():
    """the island references in the order of their ranges: short, long, class-0, paired"""
    c = reads()
    return np.concatenate([c["short_refs"], c["long_refs"], c["c0_refs"], c["pair_refs"]])


def _island_ranges(refs):
    n = len(refs)
    return dict(rid=np.asarray(refs, np.int32), loc=np.full(n, ISLAND_LO, np.int32), len=np.full(n, ISLAND_HI - ISLAND_LO, np.int32),
                strand=np.asarray([(1, -1, 0)[i % 3] for i in range(n)], np.int32))


@functools.lru_cache(maxsize=None)
def ranges(placement=None):
    """The deck: len(WIDTHS) * COPIES ranges on the bulk references, then the islands' (island_refs' order)."""
    if placement is not None:
        import far_deck
        return far_deck.place_ranges(ranges(), placement)
    for seed in range(5, 200):
        rng = np.random.default_rng(seed)
        width = rng.permutation(np.repeat(np.asarray(WIDTHS, np.int64), COPIES))
        off = np.concatenate([[0], np.cumsum(width[:-1])])
        if all(set((off[width == w] & 3).tolist()) == {0, 1, 2, 3} for w in WIDTHS):
            break
    else:
        raise AssertionError("no order in which every width meets all four values of out_off & 3")
    n = len(width)
    rid = rng.integers(0, len(BULK_REFS), n)
    L = np.asarray(BULK_REFS, np.int64)[rid]
    loc = (rng.random(n) * (L - width)).astype(np.int64)
    strand = rng.choice(np.asarray([1, -1, 0]), n)
    loc[0] = 0                                                   # at a reference's first base
    loc[1] = L[1] - width[1]                                     # ends on a reference's last base
    wide = np.flatnonzero(width >= 63)
    loc[wide[2:5]] = -3                                          # hang over a reference's first base ...
    loc[wide[5:8]] = L[wide[5:8]] - width[wide[5:8]] + 5         # ... and over its last
    for w in (1, 64, 257, 2048):                                 # duplicates
        k = np.flatnonzero(width == w)[-3:]
        rid[k[1:]], loc[k[1:]] = rid[k[0]], loc[k[0]]
    bulk = dict(rid=rid.astype(np.int32), loc=loc.astype(np.int32), len=width.astype(np.int32), strand=strand.astype(np.int32))
    isl = _island_ranges(island_refs())
    return {k: np.concatenate([bulk[k], isl[k]]) for k in bulk}


N_BULK_RANGES = len(WIDTHS) * COPIES


def tiles_of(rg, tile_cells, binsize=1):
    """work items per range of a plan with `tile_cells` cells a tile (bamCount, tile_cells None: one per range)"""
    w = np.asarray(rg["len"], np.int64)
    if tile_cells is None:
        return (w > 0).astype(np.int64)
    cells = (w + binsize - 1) // binsize
    return (cells + tile_cells - 1) // tile_cells


def cut(tile_cells, residue, binsize=1):
    """The deck without the last k of its bulk ranges, k the smallest that leaves tiles numbering `residue` modulo 8 (all
    islands stay in: their ranges are whole multiples of most tile sizes); returns (ranges, k)."""
    rg = ranges()
    per = tiles_of(rg, tile_cells, binsize)
    total = int(per.sum())
    dropped = np.concatenate([[0], np.cumsum(per[:N_BULK_RANGES][::-1])])
    k = int(np.flatnonzero((total - dropped) % 8 == residue)[0])
    assert k < 64, (tile_cells, residue, k)
    keep = np.r_[0:N_BULK_RANGES - k, N_BULK_RANGES:len(per)]
    return {key: v[keep] for key, v in rg.items()}, k


def cut_expected(name, k):
    """expected(name) for a cut that dropped the last k bulk ranges"""
    want, off = expected(name)
    return np.concatenate([want[:off[N_BULK_RANGES - k]], want[off[N_BULK_RANGES]:]])


@functools.lru_cache(maxsize=None)
def sum_ranges(placement=None):
    """Ranges of one width for the sums: the islands' and 60 on the bulk references, strands mixed."""
    if placement is not None:
        import far_deck
        return far_deck.place_ranges(sum_ranges(), placement)
    rng = np.random.default_rng(77)
    n = 60
    rid = rng.integers(0, len(BULK_REFS), n)
    loc = (rng.random(n) * (np.asarray(BULK_REFS)[rid] - SUM_WIDTH)).astype(np.int64)
    loc[:2] = (-5, 0)
    isl = _island_ranges(island_refs())
    bulk = dict(rid=rid.astype(np.int32), loc=loc.astype(np.int32), len=np.full(n, SUM_WIDTH, np.int32),
                strand=rng.choice(np.asarray([1, -1, 0], np.int32), n))
    return {k: np.concatenate([bulk[k], isl[k]]) for k in bulk}


# ---------------------------------------------------------------------------------------------------------------
# expected values (computed once per parameter set, shared and never written to)
# ---------------------------------------------------------------------------------------------------------------
def _binned(v, b):
    return np.add.reduceat(v, np.arange(0, len(v), b)) if len(v) else np.zeros(0, np.int64)


def _coverage(rg, binsize, ss, placement=None):
    """per-base oracle coverage (all reads, or forward and reverse reads apart: the sense row counts the reads on the
    range's strand, '*' = '+'), summed over bins, in the plan's flat layout; returns (flat int64, offsets)"""
    from oracle import oracle_c
    c = _reads(placement)

    def per_base(mask):
        out, off = oracle_c.coverage_core(oracle_reads(mask, placement), rg)
        return [out[off[i]:off[i + 1]].astype(np.int64) for i in range(len(off) - 1)]
    if not ss:
        parts = [_binned(v, binsize) for v in per_base(None)]
    else:
        fwd = (c["flag"] & 16) == 0
        parts = []
        for i, (f, r) in enumerate(zip(per_base(fwd), per_base(~fwd))):
            sense, anti = (r, f) if rg["strand"][i] < 0 else (f, r)
            parts.append(np.stack([_binned(sense, binsize), _binned(anti, binsize)]).T.reshape(-1))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), off


def _expected(entry, args, rg, placement=None):
    from oracle import oracle_c
    if entry == "pileup":
        out, off = oracle_c.pileup_core(oracle_reads(None, placement), rg, **args)
    else:
        out, off = _coverage(rg, args["binsize"], args["ss"], placement)
        assert out.max(initial=0) < 2 ** 31
        out = out.astype(np.int32)
    out.setflags(write=False)
    return out, off


@functools.lru_cache(maxsize=None)
def expected(name, placement=None):
    """(flat int32 result, offsets per range) of PARAM_SETS[name] on the whole deck; a cut's is its prefix"""
    return _expected(*PARAM_SETS[name], _ranges(placement), placement)


@functools.lru_cache(maxsize=None)
def expected_sum(name, placement=None):
    """the int64 sum over SUM_RANGES of what the oracle gives per range (cell 2 * bin + antisense with strands)"""
    entry, args = SUM_SETS[name]
    rg = _sum_ranges(placement)
    out, _ = _expected(entry, args, rg, placement)
    s = out.astype(np.int64).reshape(len(rg["len"]), -1).sum(axis=0)
    s.setflags(write=False)
    return s


def gpu_args(name):
    """make_params' arguments for a parameter set (mode, keywords)"""
    from bamsignals_amd import _lib
    entry, args = {**PARAM_SETS, **SUM_SETS}[name]
    a = dict(args)
    if entry == "pileup":
        mode = _lib.MODE_COUNT if a["binsize"] < 0 else _lib.MODE_PROFILE
        return mode, a
    if a["binsize"] == 1 and not a["ss"]:
        return _lib.MODE_COVERAGE, {}
    return _lib.MODE_COVERAGE_EX, a


# ---------------------------------------------------------------------------------------------------------------
# the reductions over ranges (tests/test_reduction_forms_gpu.py): the oracle's per-base cells of the deck's ranges, reduced
# in numpy by the reductions' own expected sides (tests/*_expected.py), once per parameter set; never a GPU plan
# ---------------------------------------------------------------------------------------------------------------
XCORR_MAX_LAG = 2047
# the fragment-length histogram's shapes, by whether the pair table still fits LDS beside the rows (tlen_filter, len_bin):
# 16,384 rows leave it no room
FRAG_SHAPES = {0: ((0, 16383), 1), 1: ((100, 400), 7)}
THRESHOLDS = (1, 2, 3, 5, 8, 13, 50, 1000)       # (5' ends reach 15 a cell on the deck, coverage 1,397)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _xcorr_full(mapqual, placement=None):
    import crosscorr_expected as xe
    cross, mom = xe.expected(oracle_reads(None, placement), _ranges(placement), XCORR_MAX_LAG, mapqual=mapqual)
    return _frozen(cross), _frozen(mom)


def expected_xcorr(max_lag, mapqual=0, placement=None):
    """cross[0 .. max_lag], then the five moments: lag d's sum does not depend on the largest lag asked for, so the
    result for XCORR_MAX_LAG, computed once, holds every smaller one as a prefix"""
    cross, mom = _xcorr_full(mapqual) if placement is None else _xcorr_full(mapqual, placement)
    assert 0 <= max_lag <= XCORR_MAX_LAG
    return np.concatenate([cross[:max_lag + 1], mom])


def _some_ranges(which, placement=None):
    rg = _ranges(placement)
    if which == "all":
        return rg
    c = _reads(placement)
    keep = np.isin(rg["rid"], c[{"c0": "c0_refs", "paired": "pair_refs"}[which]])
    return {k: v[keep] for k, v in rg.items()}


@functools.lru_cache(maxsize=None)
def expected_frag(tlen_filter, len_bin, midpoint, which="all", placement=None):
    """the fragment-length histogram of the deck's ranges (which: all, or the class-0 / the paired islands' alone).  No
    template of the deck is longer than 600, which one oracle bamCount over all longer lengths confirms: the rows above
    600 are zero without an oracle call each."""
    import fragsizes_expected as fe
    orc, rg = oracle_reads(None, placement), _some_ranges(which, placement)
    lo, hi = tlen_filter
    if hi <= 600 * len_bin:
        return _frozen(fe.expected(orc, rg, (lo, hi), len_bin, midpoint))
    assert len_bin == 1 and fe.whole_count(orc, rg, (601, hi), midpoint) == 0
    hist = np.zeros(fe.n_rows((lo, hi), len_bin), np.int64)
    hist[:601] = fe.expected(orc, rg, (lo, 600), len_bin, midpoint)
    return _frozen(hist)


@functools.lru_cache(maxsize=None)
def reduction_cells(signal, ss, mapqual=0, placement=None):
    """all per-base cells of the deck's ranges in the oracle's order: "coverage", or "ends" (5' ends, shift 0)"""
    import depthhist_expected as de
    return _frozen(de.cells(oracle_reads(None, placement), _ranges(placement), signal, ss, mapqual=mapqual))


def _cells(signal, ss, mapqual, placement):
    return reduction_cells(signal, ss, mapqual) if placement is None else reduction_cells(signal, ss, mapqual, placement)


@functools.lru_cache(maxsize=None)
def expected_hist(signal, ss, max_value, mapqual=0, placement=None):
    import depthhist_expected as de
    return _frozen(de.from_cells(_cells(signal, ss, mapqual, placement), max_value))


@functools.lru_cache(maxsize=None)
def expected_summary(signal, ss, thresholds, mapqual=0, placement=None):
    import summary_expected as se
    return _frozen(se.from_cells(_cells(signal, ss, mapqual, placement), _ranges(placement), ss, thresholds))


@functools.lru_cache(maxsize=None)
def expected_scaled(signal, ss, n_bins, mapqual=0, placement=None):
    import scaled_expected as sc
    return _frozen(sc.from_cells(_cells(signal, ss, mapqual, placement), _ranges(placement), ss, n_bins))


# ---------------------------------------------------------------------------------------------------------------
# the later forms (tests/test_later_forms_gpu.py): keepDup's capped cells, the V-plot and the resized coverage -- the
# oracle's cells put together by the kinds' own expected sides (tests/*_expected.py), once per parameter set; never a GPU plan
# ---------------------------------------------------------------------------------------------------------------
# the V-plot's shapes on sum_ranges() (tlen_filter, len_bin, binsize) -> rows x cols = tf1 // len_bin + 1 by ceil(2,048 /
# binsize) cells: a small table, one of exactly the 40,960 counters a gfx950 workgroup may declare (160 KiB), one row
# fewer and one row more.  No template of the deck is longer than 600.
VPLOT_SHAPES = {"small": ((0, 600), 7, 50), "budget": ((100, 399), 20, 1), "below": ((100, 379), 20, 1), "above": ((100, 419), 20, 1)}
VPLOT_CELLS = {"small": 86 * 41, "budget": 20 * 2048, "below": 19 * 2048, "above": 21 * 2048}


@functools.lru_cache(maxsize=None)
def capped_cells(shift=0, mapqual=0, placement=None):
    """per range of the deck the (2, w) int64 matrix of its per-base 5'-end cells, rows sense and antisense, uncapped"""
    import capped_expected as ce
    return tuple(_frozen(c) for c in ce.stranded_cells(oracle_reads(None, placement), _ranges(placement), shift=shift, mapqual=mapqual))


@functools.lru_cache(maxsize=None)
def expected_capped(k, binsize, ss, shift=0, mapqual=0, placement=None):
    """(flat int64 cells, offsets) of keepDup = k over ranges(): capped first, binned second (binsize -1: bamCount), the
    strands added last"""
    import capped_expected as ce
    cells = capped_cells(shift, mapqual) if placement is None else capped_cells(shift, mapqual, placement)
    flat, off = ce.ends_from_cells(cells, k, binsize, ss)
    return _frozen(flat), _frozen(off)


@functools.lru_cache(maxsize=None)
def expected_capped_cover(k, L, binsize, ss, mapqual=0, placement=None):
    """(flat int64 cells, offsets) over ranges() of the coverage of the kept reads resized to L bases"""
    import capped_expected as ce
    flat, off = ce.coverage(oracle_reads(None, placement), _ranges(placement), k, L, binsize, ss, mapqual=mapqual)
    return _frozen(flat), _frozen(off)


def capped_cover_rows(L):
    """the pairs in every range's scratch row of a capped coverage plan: the range widened by L - 1 bases on both sides,
    less what lies below base 0 (csrc/planmath.h: capped_widen; 0 for a range without width)"""
    rg = ranges()
    loc, w = rg["loc"].astype(np.int64), rg["len"].astype(np.int64)
    lo = np.maximum(loc - (L - 1), 0)
    return np.where(w > 0, np.maximum(loc - lo + w + L - 1, 0), 0)


def _some_sum_ranges(which, placement=None):
    rg = _sum_ranges(placement)
    if which == "all":
        return rg
    c = _reads(placement)
    keep = np.isin(rg["rid"], c[{"c0": "c0_refs", "paired": "pair_refs"}[which]])
    return {k: v[keep] for k, v in rg.items()}


@functools.lru_cache(maxsize=None)
def expected_vplot(tlen_filter, len_bin, binsize, midpoint, mapqual=0, which="all", placement=None):
    """the (rows, cols) int64 V-plot of sum_ranges() (which: all, or the class-0 / the paired islands' ranges alone): one
    oracle bamProfile per non-empty row band, summed over the ranges"""
    import vplot_expected as ve
    assert tlen_filter[1] <= 600
    return _frozen(ve.expected(oracle_reads(None, placement), _some_sum_ranges(which, placement), tlen_filter, len_bin, binsize, midpoint, mapqual=mapqual))


@functools.lru_cache(maxsize=None)
def resized_columns(L, placement=None):
    """the deck's read columns with every read resized to L bases from its 5' end (tests/resized_expected.py)"""
    import resized_expected as rx
    return rx.resize_columns(_reads(placement), L)


@functools.lru_cache(maxsize=None)
def expected_resized(L, pset, placement=None):
    """(flat int32 result, offsets) of the coverage parameter set PARAM_SETS[pset] on the whole deck with the reads
    resized to L bases: the oracle's coverage of the resized columns"""
    import resized_expected as rx
    entry, args = PARAM_SETS[pset]
    assert entry == "coverage"
    cols = resized_columns(L) if placement is None else resized_columns(L, placement)
    out, off = rx.coverage(cols, _ranges(placement), args["binsize"], args["ss"])
    assert out.max(initial=0) < 2 ** 31
    out = out.astype(np.int32)
    out.setflags(write=False)
    return out, off


@functools.lru_cache(maxsize=None)
def expected_resized_sum(L, ss, placement=None):
    """the int64 sum over sum_ranges() of the per-base coverage of the reads resized to L bases (cell 2 * base + antisense
    with strands)"""
    import resized_expected as rx
    rg = _sum_ranges(placement)
    per_range, _ = rx.coverage(resized_columns(L) if placement is None else resized_columns(L, placement), rg, 1, ss)
    return _frozen(per_range.reshape(len(rg["len"]), -1).sum(axis=0).astype(np.int64))
