"""GPU: the resident layout byte for byte.  Every case makes reads resident, saves them (Reads.save writes the layout as
it lies in HBM), parses the file with tests/layout_expected.py: read_layout and compares every header field, every
column over its full capacity (so the padding must be zero), every bucket index, the pair table and the device-side
checksum with the numpy restatement of csrc/bsig_types.h (layout_expected.expected_layout / expected_checksum).

The ten kernels behind it (csrc/kernels.hip: k_cigar_end, k_pair_sample, k_pair_compact, k_codemap_fill, k_span_hist,
k_chunk_scan, k_scatter, k_build_idx, k_checksum; k_check_idx on load) are otherwise seen only through results, which
an index that is too wide, a partition that is not stable among equal positions or a wrong pair-table tie leave intact.
Every case asserts that its input reaches the edge it is named for."""
import functools
import os
import tempfile

import numpy as np
import pytest

import layout_expected as le

pytestmark = pytest.mark.gpu

STAMP = "layout-pin"
MIXED_REFS = (200_000, 70_000, 150_000)
FLAGS = np.asarray([0, 16, 99, 147, 83, 163, 0x400, 0x410])
MAPQS = np.asarray([0, 10, 30, 60, 255])
SIZES = (1, 3, 255, 256, 257, 2047, 2048, 2049, 6145)        # passes of 256 reads, chunks of 2,048, the last one partial or full


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def columns(ref_len, rid, pos, span, flag, mapq, tlen):
    """the column dict of reads given in (rid, pos) order"""
    rid, pos = np.asarray(rid, np.int64), np.asarray(pos, np.int64)
    return dict(ref_len=np.asarray(ref_len, np.int32),
                ref_off=np.searchsorted(rid, np.arange(len(ref_len) + 1)).astype(np.int64),
                pos=pos.astype(np.int32), end=(pos + np.asarray(span, np.int64) - 1).astype(np.int32),
                flag=np.asarray(flag).astype(np.uint16), mapq=np.asarray(mapq).astype(np.uint8),
                tlen=np.asarray(tlen).astype(np.int32))


def spans_of_kind(rng, kind):
    """a span for each read's intended class -- 0: short with flag bit 12 (never packed), 4: short (packed when its
    pair has a code), 1, 2, 3: by span -- a twentieth of them on the class's own borders"""
    lo = np.asarray([1, 257, 4097, 65_537, 1])[kind]
    hi = np.asarray([256, 4096, 65_536, 70_000, 256])[kind]
    span = rng.integers(lo, hi + 1)
    edge = rng.random(len(kind)) < 0.05
    return np.where(edge, np.where(rng.random(len(kind)) < 0.5, lo, hi), span)


def mixed_reads(n, seed, ref_len=MIXED_REFS, weights=(0.15, 0.10, 0.05, 0.02, 0.68)):
    """n sorted reads over `ref_len`, the five classes mixed (the first five reads take one class each), equal positions
    among them, flags, mapq and tlen seeded"""
    rng = np.random.default_rng(seed)
    gstart = np.concatenate([[0], np.cumsum(ref_len)])
    g = np.sort(rng.integers(0, gstart[-1], n))
    dup = np.flatnonzero(rng.random(n) < 0.3)
    g[dup] = g[np.maximum(dup - 1, 0)]                               # equal positions: what a stable partition keeps in order
    g = np.sort(g)
    rid = np.searchsorted(gstart, g, side="right") - 1
    kind = rng.choice(5, n, p=weights)
    kind[:min(n, 5)] = rng.permutation(5)[:min(n, 5)]
    flag = FLAGS[rng.integers(0, len(FLAGS), n)]
    flag = np.where(kind == 0, flag | 0x1000, flag)
    return columns(ref_len, rid, g - gstart[rid], spans_of_kind(rng, kind), flag, MAPQS[rng.integers(0, len(MAPQS), n)],
                   rng.integers(-1000, 1001, n))


M_, I_, D_, N_, S_, H_, P_, EQ_, X_ = range(9)


def cigars_for(cols, seed):
    """CIGARs for the reads of `cols`, eight shapes in turn: one M; all nine defined ops; the undefined op codes 9 .. 15
    between two Ms; 0x4 set on a read with a CIGAR; an empty CIGAR; S / I / H / P alone; two ops; D and N alone.  Returns
    (flag, cigar_off, cigar, shape): shapes 3 .. 5 make a one-base read of whatever span the read had."""
    rng = np.random.default_rng(seed)
    span = cols["end"].astype(np.int64) - cols["pos"] + 1
    flag = cols["flag"].copy()
    ops, off = [], [0]

    def split(total, k):
        """k positive lengths that sum to total (total >= k)"""
        cuts = np.sort(rng.choice(np.arange(1, total), k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
        return np.diff(np.concatenate([[0], cuts, [total]])).tolist()
    shape = np.arange(len(span)) % 8
    for i, s in enumerate(span.tolist()):
        sh = int(shape[i])
        if sh == 1 and s >= 5:
            m, d, nn, eq, x = split(s, 5)
            one = [(3, S_), (m, M_), (4, I_), (d, D_), (nn, N_), (eq, EQ_), (x, X_), (2, P_), (7, H_)]
        elif sh == 2 and s >= 2:
            a, b = split(s, 2)
            one = [(a, M_)] + [(int(rng.integers(1, 300)), op) for op in range(9, 16)] + [(b, M_)]
        elif sh == 3:
            flag[i] |= 4
            one = [(50, M_), (10, D_)]
        elif sh == 4:
            one = []
        elif sh == 5:
            one = [(5, S_), (3, I_), (9, H_), (1, P_)]
        elif sh == 6 and s >= 2:
            a, b = split(s, 2)
            one = [(a, EQ_), (6, I_), (b, X_)]
        elif sh == 7 and s >= 2:
            a, b = split(s, 2)
            one = [(8, S_), (a, D_), (b, N_)]
        else:
            shape[i] = 0
            one = [(s, M_)]
        ops += [ln << 4 | op for ln, op in one]
        off.append(len(ops))
    return flag, np.asarray(off, np.int64), np.asarray(ops, np.uint32), shape


# ---------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from bamsignals_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def resident(ctx, cols, end=True, cigar=None):
    from bamsignals_amd.device import Reads
    if cigar is not None:
        flag, cigar_off, cg = cigar
        return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], flag, cols["mapq"], cols["tlen"], cigar_off=cigar_off, cigar=cg)
    return Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])


def saved_layout(reads):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.bsig")
        reads.save(path, STAMP)
        got = le.read_layout(path)
    assert got["stamp"] == STAMP
    return got


def want_layout(cols, **knobs):
    return le.expected_layout(cols["ref_len"], cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"], **knobs)


def assert_layout(reads, cols, want=None, **knobs):
    """The layout `reads` holds on the device is the restatement's of `cols` (knobs: bucket_reads, pack -- what the
    process's BAMSIGNALS_BUCKET_READS and BAMSIGNALS_PACK say), in every header field, column, index, the pair table and
    the checksum, and reads.info() says the same.  Returns (the file's layout, the restated one)."""
    want = want_layout(cols, **knobs) if want is None else want
    got = saved_layout(reads)
    bad = le.layout_differences(got, want)
    info = {k: v for k, v in reads.info().items() if k != "hbm_bytes"}
    if info != le.expected_info(want):
        bad.append("info(): %r, expected %r" % (info, le.expected_info(want)))
    assert not bad, "the layout differs from the restatement:\n  " + "\n  ".join(bad)
    return got, want


def check(ctx, cols, want=None, cigar=None, **knobs):
    r = resident(ctx, cols, cigar=cigar)
    try:
        return assert_layout(r, cols, want, **knobs)
    finally:
        r.close()


def class_counts(want):
    return [C["n"] for C in want["cls"]]


# ---------------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["end", "cigar"])
@pytest.mark.parametrize("n", SIZES)
def test_read_counts(ctx, n, how):
    cols = mixed_reads(n, 1000 + n)
    assert len(cols["pos"]) == n
    if how == "cigar":
        flag, off, cg, shape = cigars_for(cols, 2000 + n)
        end = le.cigar_end(cols["pos"], flag, off, cg)
        span0 = cols["end"].astype(np.int64) - cols["pos"] + 1
        one_base = np.isin(shape, (3, 4, 5))
        assert np.array_equal((end - cols["pos"] + 1)[~one_base], span0[~one_base]) and np.all(end[one_base] == cols["pos"][one_base])
        if n >= 255:
            # every shape is there: all nine ops, the op codes 9 .. 15, 0x4, the empty CIGAR, S / I / H / P alone
            assert set(shape.tolist()) == set(range(8)) and set((cg & 15).tolist()) == set(range(16))
            assert np.any(np.diff(off) == 0) and np.any((flag & 4) != 0)
        cols = dict(cols, flag=flag, end=end.astype(np.int32))
        _, want = check(ctx, cols, cigar=(flag, off, cg))
    else:
        _, want = check(ctx, cols)
    assert sum(class_counts(want)) == n
    assert sum(c > 0 for c in class_counts(want)) == min(n, 5), class_counts(want)      # mixed classes at every size


# ---------------------------------------------------------------------------------------------------------------
# span edges, empty classes, one class alone
# ---------------------------------------------------------------------------------------------------------------
EDGE_SPANS = (1, 256, 257, 4096, 4097, 65_536, 65_537)


def edge_reads(spans, with_high_flags=True, seed=7):
    rng = np.random.default_rng(seed)
    span, flag = [], []
    for s in spans:
        span += [s] * 40
        flag += FLAGS[rng.integers(0, len(FLAGS), 40)].tolist()
        if with_high_flags and s in (256, 257, 4096):
            span += [s] * 12
            flag += [4096, 4096 | 16, 0x8000, 0xFFFF] * 3
    n = len(span)
    order = rng.permutation(n)
    g = np.sort(rng.integers(0, 280_000, n))
    g[1::3] = g[0:-1:3][:len(g[1::3])]                          # equal positions
    gstart = np.concatenate([[0], np.cumsum(MIXED_REFS)])
    rid = np.searchsorted(gstart, g, side="right") - 1
    return columns(MIXED_REFS, rid, g - gstart[rid], np.asarray(span)[order], np.asarray(flag)[order],
                   MAPQS[rng.integers(0, len(MAPQS), n)], rng.integers(-500, 501, n))


@pytest.mark.parametrize("case", ["all_edges", "class_3_empty", "class_2_alone", "packed_alone", "class_0_alone"])
def test_span_edges(ctx, case):
    if case == "all_edges":
        cols = edge_reads(EDGE_SPANS)
    elif case == "class_3_empty":
        cols = edge_reads(EDGE_SPANS[:-1])
    elif case == "class_2_alone":
        cols = edge_reads((4097, 5000, 65_536), with_high_flags=False)
    elif case == "packed_alone":
        cols = edge_reads((1, 100, 256), with_high_flags=False)
    else:
        cols = edge_reads((1, 100, 256), with_high_flags=False)
        cols["flag"] = cols["flag"] | np.uint16(0x2000)
    _, want = check(ctx, cols)
    span = cols["end"].astype(np.int64) - cols["pos"] + 1
    cls, n = want["read_class"], class_counts(want)
    high = cols["flag"] >= 4096
    if case in ("all_edges", "class_3_empty"):
        # a flag above the SAM bits: span 256 stays in class 0, spans 257 and 4,096 go to class 2 (class 1's word has 12 flag bits)
        for s, c in ((256, 0), (257, 2), (4096, 2)):
            assert np.sum(high & (span == s)) == 12 and np.all(cls[high & (span == s)] == c)
        for s, c in ((1, 4), (256, 4), (257, 1), (4096, 1), (4097, 2), (65_536, 2)):
            assert np.all(cls[~high & (span == s)] == c) and np.any(~high & (span == s))
        assert [C["maxspan"] for C in want["cls"]][:3] == [256, 4096, 65_536] and want["cls"][4]["maxspan"] == 256
    if case == "all_edges":
        assert np.all(cls[span == 65_537] == 3) and all(n) and want["cls"][3]["maxspan"] == 65_537
    elif case == "class_3_empty":
        assert n[3] == 0 and all(n[c] for c in (0, 1, 2, 4))
    else:
        only = dict(class_2_alone=2, packed_alone=4, class_0_alone=0)[case]
        assert [c for c in range(5) if n[c]] == [only]            # the checksum's salt starts at this class


# ---------------------------------------------------------------------------------------------------------------
# chunks of many references
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_references():
    rng = np.random.default_rng(31)
    n_small = 4000
    per = rng.integers(0, 4, n_small)                                 # 0 .. 3 reads each
    length = rng.integers(300, 5000, n_small)
    length[rng.integers(0, n_small, 60)] = 0
    length[rng.integers(0, n_small, 60)] = 65_535
    length[rng.integers(0, n_small, 60)] = 65_536
    per[:25] = 0                                                      # empty references in front,
    for a in (700, 1500, 2600):
        per[a:a + 300] = 0                                            # in runs in the middle (300 > a chunk's worth of them)
    per[-40:] = 0                                                     # and at the end
    big_at = 2000
    ref_len = np.concatenate([length[:big_at], [3_000_000], length[big_at:]])
    per = np.concatenate([per[:big_at], [9000], per[big_at:]])
    n = int(per.sum())
    rid = np.repeat(np.arange(len(ref_len)), per)
    pos = np.empty(n, np.int64)
    for r in np.flatnonzero(per):
        lo = int(np.searchsorted(rid, r))
        pos[lo:lo + per[r]] = np.sort(rng.integers(0, max(int(ref_len[r]), 1), per[r]))
    kind = rng.choice(5, n, p=(0.15, 0.10, 0.05, 0.02, 0.68))
    flag = FLAGS[rng.integers(0, len(FLAGS), n)]
    flag = np.where(kind == 0, flag | 0x1000, flag)
    return columns(ref_len, rid, pos, spans_of_kind(rng, kind), flag, MAPQS[rng.integers(0, len(MAPQS), n)], rng.integers(-1000, 1001, n))


def test_many_references_in_a_chunk(ctx):
    cols = many_references()
    n, ref_off, ref_len = len(cols["pos"]), cols["ref_off"], cols["ref_len"]
    rid = np.searchsorted(ref_off[1:], np.arange(n), side="right")
    per = np.diff(ref_off)
    chunk_first, chunk_last = rid[::le.CHUNK], rid[np.minimum(np.arange(le.CHUNK - 1, n + le.CHUNK - 1, le.CHUNK), n - 1)]
    refs_in_chunk = chunk_last - chunk_first + 1
    assert np.any(refs_in_chunk == 1) and np.any(refs_in_chunk >= 300), refs_in_chunk          # inside one reference | hundreds
    assert per[0] == 0 and per[-1] == 0 and n > 3 * le.CHUNK
    # an empty run inside a chunk: some chunk's references include a run of >= 300 without reads
    empty_run = np.flatnonzero(per[700:1000] == 0)
    assert len(empty_run) == 300 and np.any((chunk_first < 700) & (chunk_last >= 1000))
    units = (ref_len.astype(np.int64) >> 16) + 1
    for L, u in ((0, 1), (65_535, 1), (65_536, 2)):
        assert np.any(ref_len == L) and np.all(units[ref_len == L] == u)
    assert np.any(per[ref_len == 65_536] > 0) and np.any(per[ref_len == 65_535] > 0)
    _, want = check(ctx, cols)
    assert all(class_counts(want))


# ---------------------------------------------------------------------------------------------------------------
# positions outside the reference
# ---------------------------------------------------------------------------------------------------------------
def test_positions_outside_the_reference(ctx):
    rng = np.random.default_rng(41)
    ref_len = np.asarray([70_000, 1000, 65_536, 40_000])
    units = (ref_len >> 16) + 1
    rid, pos = [], []
    for r, L in enumerate(ref_len):
        bp = int(units[r]) << 16
        inside = np.sort(rng.integers(0, L, 300))
        below = np.sort(rng.integers(-5000, 0, 20))
        beyond = np.sort(np.concatenate([[bp, bp, bp + 1], rng.integers(bp, bp + 100_000, 20)]))
        slack = np.sort(rng.integers(L, bp, 10))                      # past the reference's end, inside its last unit: may be packed
        p = np.concatenate([below, np.sort(np.concatenate([inside, slack])), beyond])
        rid += [r] * len(p)
        pos.append(p)
    pos = np.concatenate(pos)
    n = len(pos)
    cols = columns(ref_len, rid, pos, rng.integers(1, 257, n), FLAGS[rng.integers(0, 2, n)], np.full(n, 30), np.zeros(n))
    _, want = check(ctx, cols)
    ref_bp = (units << 16)[np.asarray(rid)]
    outside = (pos < 0) | (pos >= ref_bp)
    cls = want["read_class"]
    assert np.sum(pos < 0) == 80 and np.sum(pos >= ref_bp) == 92 and np.sum(pos == ref_bp) == 8
    assert np.all(cls[outside] == 0) and np.all(cls[~outside] == 4)                  # short reads all; outside: never packed
    C0 = want["cls"][0]
    assert np.array_equal(C0["pos"][:C0["n"]], pos[outside])                        # the column holds the position unclamped
    g = (want["ref_unit0"].astype(np.int64)[np.asarray(rid)] << 16) + np.clip(pos, 0, ref_bp - 1)
    assert np.array_equal(le.read_buckets(want, 0), (g >> C0["kshift"])[outside])   # the index files it under the clamped one


# ---------------------------------------------------------------------------------------------------------------
# the chunk scan beyond 1,024 chunks; the pair table's sample beyond 2,047
# ---------------------------------------------------------------------------------------------------------------
SCAN_REFS = (3_000_000, 0, 1_000_000)
UNSAMPLED_PAIR = (0x20, 77)          # (flag, mapq) on short reads of odd chunks only: no code at a sampling stride of 2
LONG_ONLY_PAIR = (0x40, 78)          # ... on reads of span > 256 only: never counted


@functools.lru_cache(maxsize=2)
def scan_reads(n):
    rng = np.random.default_rng(n)
    gstart = np.concatenate([[0], np.cumsum(SCAN_REFS)])
    g = np.sort(rng.integers(0, gstart[-1], n))
    rid = np.searchsorted(gstart, g, side="right") - 1
    # every chunk holds every class: a seeded pattern of 64 kinds that has all five, repeated
    pattern = np.concatenate([[0, 1, 2, 3, 4], rng.choice(5, 59, p=(0.15, 0.10, 0.05, 0.02, 0.68))])
    kind = pattern[(np.arange(n) + rng.integers(0, 64, n // le.CHUNK + 1)[np.arange(n) // le.CHUNK]) % 64]
    flag = FLAGS[rng.integers(0, len(FLAGS), n)]
    flag = np.where(kind == 0, flag | 0x1000, flag)
    mapq = MAPQS[rng.integers(0, len(MAPQS), n)]
    span = spans_of_kind(rng, kind)
    i = np.arange(n)
    odd = ((i // le.CHUNK) % 2 == 1) & (kind == 4) & (i % 3 == 0)
    flag[odd], mapq[odd] = UNSAMPLED_PAIR
    lng = (kind == 1) & (i % 2 == 0)
    flag[lng], mapq[lng] = LONG_ONLY_PAIR
    cols = columns(SCAN_REFS, rid, g - gstart[rid], span, flag, mapq, rng.integers(-1000, 1001, n))
    return cols, want_layout(cols)


@pytest.mark.parametrize("n_chunks", [1025, 3000])
def test_scan_beyond_1024_chunks(ctx, n_chunks):
    n = (n_chunks - 1) * le.CHUNK + 1 if n_chunks == 1025 else n_chunks * le.CHUNK - 777
    cols, want = scan_reads(n)
    assert n == len(cols["pos"]) and (n + le.CHUNK - 1) // le.CHUNK == n_chunks
    per = (n_chunks + 1023) // 1024
    assert per == (2 if n_chunks == 1025 else 3)
    idle = 1024 - (n_chunks + per - 1) // per
    first_past = ((n_chunks + per - 1) // per + 1) * per              # the second idle thread's first chunk
    assert (idle, first_past > n_chunks) == ((511, True) if n_chunks == 1025 else (24, True))
    full = n // le.CHUNK
    seen = np.bincount((np.arange(full * le.CHUNK) // le.CHUNK) * 5 + want["read_class"][:full * le.CHUNK], minlength=full * 5)
    assert seen.min() > 0                                             # all five classes in every full chunk, so in every slab
    check(ctx, cols, want)


def test_pair_table_sampling_stride_2(ctx):
    cols, want = scan_reads(3000 * le.CHUNK - 777)
    n = len(cols["pos"])
    assert n > 2_000_000 and le.sample_stride(n) == 2 and le.sample_stride(2047 * le.CHUNK) == 1
    key = cols["flag"].astype(np.int64) | cols["mapq"].astype(np.int64) << 12
    span = cols["end"].astype(np.int64) - cols["pos"] + 1
    table = (want["fmtab"][:want["n_codes"]].astype(np.int64) & 0xFFF) | (want["fmtab"][:want["n_codes"]].astype(np.int64) >> 16) << 12
    for (f, q), where in ((UNSAMPLED_PAIR, span <= 256), (LONG_ONLY_PAIR, span > 256)):
        k = f | q << 12
        assert np.sum(key == k) > 100_000 and np.all(where[key == k]) and k not in table.tolist()
        assert not np.any(want["read_class"][key == k] == 4)
    # ... while a rarer pair of the sampled chunks has its code: the unsampled pair would be among the most frequent
    counts = np.bincount(key[span <= 256], minlength=1 << 20)
    assert counts[UNSAMPLED_PAIR[0] | UNSAMPLED_PAIR[1] << 12] > counts[table].min()
    check(ctx, cols, want)


# ---------------------------------------------------------------------------------------------------------------
# the pair table
# ---------------------------------------------------------------------------------------------------------------
def pair_reads(counts, seed, extra_long=0):
    """short reads whose (flag, mapq) pairs are len(counts) distinct seeded keys, pair j on counts[j] reads, shuffled"""
    rng = np.random.default_rng(seed)
    keys = rng.choice(1 << 20, len(counts), replace=False)
    key = rng.permutation(np.repeat(keys, counts))
    n = len(key)
    g = np.sort(rng.integers(0, 270_000, n))
    gstart = np.concatenate([[0], np.cumsum(MIXED_REFS)])
    rid = np.searchsorted(gstart, g, side="right") - 1
    span = rng.integers(1, 257, n)
    span[:extra_long] = 300
    return columns(MIXED_REFS, rid, g - gstart[rid], span, key & 0xFFF, key >> 12, rng.integers(-300, 301, n)), keys


@pytest.mark.parametrize("case", ["fewer_than_512", "exactly_512", "tie_at_the_cut", "more_than_16384", "pack_off"])
def test_pair_table(ctx, case, monkeypatch):
    knobs = {}
    if case == "fewer_than_512":
        cols, keys = pair_reads(np.arange(1, 101), 51)
    elif case == "exactly_512":
        cols, keys = pair_reads(np.full(512, 2), 52)
    elif case == "tie_at_the_cut":
        cols, keys = pair_reads(np.concatenate([np.full(500, 3), np.full(100, 2)]), 53)
    elif case == "more_than_16384":
        cols, keys = pair_reads(np.concatenate([np.arange(2, 302), np.ones(17_000, np.int64)]), 54)
    else:
        cols, keys = pair_reads(np.arange(1, 101), 55)
        monkeypatch.setenv("BAMSIGNALS_PACK", "0")
        knobs = dict(pack=False)
    got, want = check(ctx, cols, **knobs)
    tkeys, tcounts = le.pair_table(cols["pos"], cols["end"], cols["flag"], cols["mapq"])
    assert set(tkeys.tolist()) == set(keys.tolist())                  # every pair was seen on a sampled short read
    n = class_counts(want)
    key = cols["flag"].astype(np.int64) | cols["mapq"].astype(np.int64) << 12
    if case == "fewer_than_512":
        assert want["n_codes"] == 100 and n[0] == 0 and np.all(want["fmtab"][100:] == 0)
    elif case == "exactly_512":
        assert want["n_codes"] == 512 and len(tkeys) == 512 and n[0] == 0
        assert np.array_equal(tkeys, np.sort(keys))                   # all counts equal: the codes go by key alone
    elif case == "tie_at_the_cut":
        assert len(tkeys) == 600 and tcounts[511] == tcounts[512] == 2 and tcounts[499] == 3 and tcounts[500] == 2
        assert np.all(np.diff(tkeys[500:]) > 0)                       # among the equal counts the smaller keys win
        late = np.isin(key, tkeys[512:])
        assert late.sum() == 2 * 88 and np.all(want["read_class"][late] == 0) and n[0] == late.sum() and n[4] == len(key) - n[0]
    elif case == "more_than_16384":
        assert len(tkeys) > 16_384 and want["n_codes"] == 512         # more than the pair list holds: the counters come back
        assert tcounts[511] == 1 and tcounts[300] == 1 and tcounts[299] == 2
        assert n[0] == 17_000 - 212 and n[4] == len(key) - n[0]
    else:
        assert want["n_codes"] == 0 and want["fmtab"] is None and n[4] == 0 and n[0] == len(key)
        assert got["fmtab"] is None and got["cls"][4]["col_cap"] == 0


# ---------------------------------------------------------------------------------------------------------------
# bucket width
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bucket_set(name):
    if name == "dense":
        return mixed_reads(40_000, 61, ref_len=(70_000,))             # 2 units = 131,072 bp: 4.8 bp a packed read
    return mixed_reads(100, 62, ref_len=(1_000_000, 1_000_000, 1_000_000), weights=(0.2, 0.2, 0.2, 0.1, 0.3))


@pytest.mark.parametrize("value", ["1", "16", "4096", "1e12"])
@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_bucket_reads(ctx, name, value, monkeypatch):
    cols = bucket_set(name)
    monkeypatch.setenv("BAMSIGNALS_BUCKET_READS", value)
    _, want = check(ctx, cols, bucket_reads=float(value))
    k = [C["kshift"] for C in want["cls"]]
    assert all(class_counts(want))
    if (name, value) == ("dense", "1"):
        assert k[4] == 4                                              # the lower clamp
    if (name, value) == ("dense", "16"):
        assert 4 < k[4] < 15 and all(4 < k[c] < 16 for c in range(4))     # interior values in every class
    if (name, value) == ("dense", "4096"):
        assert k[4] == 14 and 16 in k[:4]
    if value == "1e12" or name == "sparse":
        assert k == [16, 16, 16, 16, 15]                              # the upper clamps: 15 for the packed class, 16 elsewhere


# ---------------------------------------------------------------------------------------------------------------
# the same bytes by every route
# ---------------------------------------------------------------------------------------------------------------
def test_same_bytes_by_every_route(ctx, tmp_path, monkeypatch):
    from bamsignals_amd import write_columns_as_bam
    from bamsignals_amd.bamio import BamFile
    from bamsignals_amd.device import Context, Reads
    from bamsignals_amd.synth import synth_reads
    c = synth_reads(200_000, [1_000_000, 400_000], seed=71, paired=True)
    # an empty reference between the two
    cols = dict(c, ref_len=np.asarray([1_000_000, 50_000, 400_000], np.int32), ref_off=np.asarray([c["ref_off"][0], c["ref_off"][1], c["ref_off"][1], c["ref_off"][2]], np.int64))
    assert np.diff(cols["ref_off"]).tolist()[1] == 0 and len(cols["pos"]) == 200_000
    assert np.array_equal(le.cigar_end(cols["pos"], cols["flag"], cols["cigar_off"], cols["cigar"]), cols["end"])
    bam = str(tmp_path / "routes.bam")
    write_columns_as_bam(bam, ["a", "b", "c"], cols)
    want = want_layout(cols)
    assert want["cls"][4]["n"] > 0 and want["cls"][1]["n"] > 0
    routes = {}

    def keep(name, r):
        path = str(tmp_path / (name + ".bsig"))
        r.save(path, STAMP)
        routes[name] = (path, le.read_layout(path))
        return r
    cigar = (cols["flag"], cols["cigar_off"], cols["cigar"])
    first = keep("end", resident(ctx, cols))
    keep("cigar", resident(ctx, cols, cigar=cigar)).close()
    other = Context(0)
    keep("clone", first.clone(other)).close()
    keep("load", Reads.load(other, routes["end"][0], STAMP)).close()
    first.close()
    bf = BamFile(bam)
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", "0")
    keep("cpu_decode", Reads.from_bam(ctx, bf)).close()
    monkeypatch.setenv("BAMSIGNALS_DEVICE_DECODE", "require")
    keep("device_decode", Reads.from_bam(ctx, bf)).close()
    monkeypatch.setenv("BAMSIGNALS_SHARD_MIN_BLOCKS", "1")
    monkeypatch.setenv("BAMSIGNALS_SHARDED_DECODE", "require")
    many, sharded = Reads.from_bam_multi([ctx, other], bf)
    assert sharded
    for k, r in enumerate(many):
        keep("shard%d" % k, r).close()
    bf.close()
    other.close()
    assert len(routes) == 8
    for name, (_, got) in routes.items():
        bad = le.layout_differences(got, want)
        assert not bad, "route %s differs from the restatement:\n  " % name + "\n  ".join(bad)
        bad = le.layout_differences(got, routes["end"][1])
        assert not bad, "route %s differs from the upload with end:\n  " % name + "\n  ".join(bad)


# ---------------------------------------------------------------------------------------------------------------
# sortedness
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sorted_set():
    """6,145 reads over four references, the second empty; no two neighbours inside a reference at one position"""
    rng = np.random.default_rng(81)
    per = [2500, 0, 2000, 1645]
    ref_len = [400_000, 5000, 300_000, 200_000]
    rid = np.repeat(np.arange(4), per)
    pos = np.concatenate([np.sort(rng.choice(np.arange(100, L), m, replace=False)) for L, m in zip(ref_len, per)])
    n = len(pos)
    kind = rng.choice(5, n, p=(0.15, 0.10, 0.05, 0.02, 0.68))
    flag = np.where(kind == 0, 0x1000, FLAGS[rng.integers(0, len(FLAGS), n)])
    return columns(ref_len, rid, pos, spans_of_kind(rng, kind), flag, MAPQS[rng.integers(0, len(MAPQS), n)], rng.integers(-1000, 1001, n))


@pytest.mark.parametrize("at", [1, 256, 2048, 4096, 6144])
def test_an_inversion_is_refused(ctx, at):
    """reads at - 1 and at exchange positions: across a 256-read pass border, a chunk border, at the file's two ends"""
    from bamsignals_amd import _lib
    cols = sorted_set()
    assert len(cols["pos"]) == 6145 and at < 6145
    rid = np.searchsorted(cols["ref_off"][1:], [at - 1, at], side="right")
    assert rid[0] == rid[1] and cols["pos"][at - 1] < cols["pos"][at]
    pos = cols["pos"].copy()
    pos[[at - 1, at]] = pos[[at, at - 1]]
    span = cols["end"] - cols["pos"]
    bad = dict(cols, pos=pos, end=pos + span)
    with pytest.raises(_lib.BsigError, match="sorted"):
        resident(ctx, bad).close()


@pytest.mark.parametrize("ref", [2, 3])
def test_a_descent_at_a_reference_start_is_accepted(ctx, ref):
    """the first read of reference 2 (behind the empty reference 1) and of reference 3 lies below its predecessor"""
    cols = sorted_set()
    i = int(cols["ref_off"][ref])
    assert np.diff(cols["ref_off"]).tolist()[1] == 0 and 0 < i < 6145
    assert cols["pos"][i] < cols["pos"][i - 1]
    check(ctx, cols)
