"""The claims of tests/forms_deck.py about its own reads and ranges, checked with the C oracle alone: the islands hold the
counts they name, their windows start at every residue modulo 8 in every class they are there for (the class-0 islands in
class 0 of both layouts, the paired islands in the packed class), the ranges meet every
value of out_off & 3 at every width, the cuts leave the tile counts they promise, every parameter set of the matrix
counts something, and no cell leaves the 16-bit tile images' range without the heavy-tile knob.  For the later forms
(tests/test_later_forms_gpu.py): cells on both sides of every cap, every branch of the capped bins' adder, scratch rows
around the capped scan's rounds, the V-plot's shapes and the resized coverage."""
import hashlib

import numpy as np

import forms_deck as deck


def test_islands_hold_their_counts():
    c = deck.reads()
    n_per_ref = np.diff(c["ref_off"])
    assert list(n_per_ref[:len(deck.BULK_REFS)]) == [deck.BULK_READS] * len(deck.BULK_REFS)
    assert sorted(c["short_m"].tolist()) == list(deck.ISLAND_COUNTS) and len(deck.ISLAND_COUNTS) == 9 + 3 * 13
    assert sorted(c["long_m"].tolist()) == list(deck.LONG_COUNTS) and max(deck.LONG_COUNTS) == 769
    assert np.array_equal(n_per_ref[c["short_refs"]], c["short_m"])
    assert np.array_equal(n_per_ref[c["long_refs"]], 2 * c["long_m"])
    isl = slice(int(c["ref_off"][len(deck.BULK_REFS)]), int(c["ref_off"][c["c0_refs"][0]]))       # the short and the long islands
    assert c["pos"][isl].min() >= deck.ISLAND_LO and c["pos"][isl].max() < deck.ISLAND_HI
    assert set(c["flag"][isl].tolist()) == {0, 16} and set(c["mapq"][isl].tolist()) == {deck.ISLAND_MAPQ}
    # the class-0 and the paired islands: the counts up to 2,049, which hold NT - 1, NT, NT + 1 and 8 NT - 1, 8 NT,
    # 8 NT + 1 for every workgroup size the reductions are built for
    assert len(deck.C0_COUNTS) == 33 and sum(deck.C0_COUNTS) == 19_047
    assert {n + d for nt in (64, 128, 256) for n in (nt, 8 * nt) for d in (-1, 0, 1)} <= set(deck.C0_COUNTS)
    span = c["end"].astype(np.int64) - c["pos"] + 1
    for refs, m, flags in ((c["c0_refs"], c["c0_m"], {0x1000, 0x1010, 0x1063, 0x1053}), (c["pair_refs"], c["pair_m"], {99, 83})):
        assert sorted(m.tolist()) == list(deck.C0_COUNTS)
        assert np.array_equal(n_per_ref[refs], m)
        assert np.all(c["ref_len"][refs] == deck.ISLAND_LEN)
        grp = slice(int(c["ref_off"][refs[0]]), int(c["ref_off"][refs[-1] + 1]))
        assert grp.stop - grp.start == 19_047
        assert c["pos"][grp].min() >= deck.ISLAND_LO and c["pos"][grp].max() < deck.ISLAND_HI
        assert span[grp].min() == 1 and span[grp].max() == 256
        assert set(c["flag"][grp].tolist()) == flags and set(c["mapq"][grp].tolist()) == {deck.ISLAND_MAPQ}
        paired = (c["flag"][grp] & 1) != 0
        a = np.abs(c["tlen"][grp].astype(np.int64))
        assert np.all((a[paired] >= 50) & (a[paired] <= 600)) and np.all(a[~paired] == 0)
        assert np.all((c["tlen"][grp][paired] < 0) == ((c["flag"][grp][paired] & 16) != 0))
    assert int(c["ref_off"][-1]) == len(c["pos"]) == 3 * deck.BULK_READS + int(c["short_m"].sum()) + 2 * int(c["long_m"].sum()) + 2 * 19_047
    # sorted by position inside every reference
    for r in range(len(c["ref_len"])):
        p = c["pos"][c["ref_off"][r]:c["ref_off"][r + 1]]
        assert np.all(np.diff(p) >= 0)
    # the bulk references: the span classes' borders, mapq's extremes, unmapped / duplicate / paired flags
    span = c["end"].astype(np.int64) - c["pos"] + 1
    bulk = slice(0, int(c["ref_off"][len(deck.BULK_REFS)]))
    for s in deck.SPAN_EDGES:
        assert np.any(span[bulk] == s), s
    assert {0, 255} <= set(c["mapq"][bulk].tolist())
    for f in (0x4, 0x400):
        assert np.any((c["flag"][bulk] & f) != 0)
    paired = (c["flag"][bulk] & 1) != 0
    assert paired.any() and np.all(c["tlen"][bulk][paired] != 0)


def test_island_classes_and_window_starts():
    c = deck.reads()
    for packed, cls_id, refs, m in ((True, 4, c["short_refs"], c["short_m"]), (False, 0, c["short_refs"], c["short_m"]),
                                    (True, 1, c["long_refs"], c["long_m"]), (True, 2, c["long_refs"], c["long_m"]),
                                    (False, 1, c["long_refs"], c["long_m"]), (False, 2, c["long_refs"], c["long_m"]),
                                    (True, 0, c["c0_refs"], c["c0_m"]), (False, 0, c["c0_refs"], c["c0_m"]),
                                    (True, 4, c["pair_refs"], c["pair_m"]), (False, 0, c["pair_refs"], c["pair_m"])):
        start, count = deck.island_windows(packed, cls_id, refs)
        assert np.array_equal(count, m), (packed, cls_id)                      # nj == m: all of them in the one class
        assert set((start[m > 0] % 8).tolist()) == set(range(8)), (packed, cls_id)
        # (which implies both parities: the dword a one-half-word-per-lane read of a 16-bit column selects from)
        assert set((start[m > 0] % 2).tolist()) == {0, 1}, (packed, cls_id)
    # the default layout packs every short island read and leaves some of the bulk's short reads in class 0
    cls = deck.read_classes(True)
    span = c["end"].astype(np.int64) - c["pos"] + 1
    assert np.any((cls == 0) & (span <= 256)) and np.any(cls == 3)
    assert not np.any(deck.read_classes(False) == 4)
    # the default layout's class 0 is the bulk's 1,098 scattered reads and the class-0 islands, whose reads no code takes
    on_c0 = np.zeros(len(cls), bool)
    on_c0[int(c["ref_off"][c["c0_refs"][0]]):int(c["ref_off"][c["c0_refs"][-1] + 1])] = True
    assert np.all(cls[on_c0] == 0) and np.all(c["flag"][on_c0] >= 4096)
    assert int(np.sum((cls == 0) & ~on_c0)) == 1098 and np.all(np.flatnonzero((cls == 0) & ~on_c0) < 3 * deck.BULK_READS)


def test_the_reads_and_ranges_in_front_of_the_new_islands_are_pinned():
    """The bulk references and the short and long islands (184,725 reads on 75 references), their 424 ranges and the sums'
    132, as they were before the class-0 and the paired islands came behind them: one digest of their columns."""
    c, rg, srg = deck.reads(), deck.ranges(), deck.sum_ranges()
    n_refs = int(c["c0_refs"][0])
    n_reads = int(c["ref_off"][n_refs])
    n_isl = len(c["short_refs"]) + len(c["long_refs"])
    assert (n_reads, n_refs, deck.N_BULK_RANGES + n_isl, 60 + n_isl) == (184_725, 75, 424, 132)
    h = hashlib.sha256()
    for k, dtype in (("pos", "<i4"), ("end", "<i4"), ("flag", "<u2"), ("mapq", "u1"), ("tlen", "<i4")):
        h.update(np.ascontiguousarray(c[k][:n_reads], dtype).tobytes())
    h.update(np.ascontiguousarray(c["ref_off"][:n_refs + 1], "<i8").tobytes())
    h.update(np.ascontiguousarray(c["ref_len"][:n_refs], "<i4").tobytes())
    for r, n in ((rg, deck.N_BULK_RANGES + n_isl), (srg, 60 + n_isl)):
        for k in ("rid", "loc", "len", "strand"):
            h.update(np.ascontiguousarray(r[k][:n], "<i4").tobytes())
    assert h.hexdigest() == "efe15b2c7c1f2331265f0a55196f2694fdf0d4f327af7518dd15b7eeb4bb3d8e"


def test_frag_expectations_count_both_island_groups():
    """what the fragment-length cases of tests/test_reduction_forms_gpu.py compare with counts first-of-pair reads of the
    class-0 islands and of the paired (packed) islands, each group taken alone, for every shape and midpoint rule"""
    for tf, len_bin in deck.FRAG_SHAPES.values():
        for mid in (False, True):
            whole = deck.expected_frag(tf, len_bin, mid)
            assert whole.dtype == np.int64 and len(whole) == tf[1] // len_bin + 1
            for which in ("c0", "paired"):
                part = deck.expected_frag(tf, len_bin, mid, which)
                assert part.any() and np.all(part <= whole), (tf, len_bin, mid, which)


def test_first_of_pair_reads_in_the_new_islands():
    """what the fragment-length histogram counts (requiredF 66: first of a proper pair) inside every class-0 and every
    paired island's range: more than nothing for m > 0, a seeded half of a class-0 island's reads, all of a paired one's"""
    c = deck.reads()
    five = np.where((c["flag"] & 16) != 0, c["end"], c["pos"])
    first = ((c["flag"] & 66) == 66) & (five >= deck.ISLAND_LO) & (five < deck.ISLAND_HI)
    for refs, m, whole in ((c["c0_refs"], c["c0_m"], False), (c["pair_refs"], c["pair_m"], True)):
        for r, k in zip(refs, m):
            seg = slice(int(c["ref_off"][r]), int(c["ref_off"][r + 1]))
            n_first = int(np.sum((c["flag"][seg] & 66) == 66))
            assert n_first == (k if whole else (k + 1) // 2), (r, k)
            assert (int(first[seg].sum()) > 0) == (k > 0), (r, k)


def test_ranges_meet_every_offset_strand_and_edge():
    rg = deck.ranges()
    nb = deck.N_BULK_RANGES
    width = rg["len"][:nb].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(width[:-1])])
    for w in deck.WIDTHS:
        assert np.sum(width == w) == deck.COPIES
        assert set((off[width == w] & 3).tolist()) == {0, 1, 2, 3}, w
    for t in deck.TILES:
        assert {t - 1, t, t + 1, 2 * t + 3} <= set(deck.WIDTHS)
    assert set(range(10)) | {63, 64, 65, 255, 256, 257} <= set(deck.WIDTHS)
    assert set(rg["strand"][:nb].tolist()) == {1, -1, 0}
    L = np.asarray(deck.BULK_REFS)[rg["rid"][:nb]]
    end = rg["loc"][:nb].astype(np.int64) + width
    assert np.any(rg["loc"][:nb] == 0) and np.any((end == L) & (width > 0))
    assert np.any(rg["loc"][:nb] < 0) and np.any(end > L)
    key = np.stack([rg["rid"][:nb], rg["loc"][:nb], rg["len"][:nb]])
    assert len(np.unique(key, axis=1).T) < nb                                  # duplicates
    # wide and one-cell tiles are neighbours in genomic order, which is the order of a plan's tiles
    order = np.lexsort((rg["loc"][:nb], rg["rid"][:nb]))
    w = width[order]
    assert np.any((w[:-1] >= 2048) & (w[1:] <= 1)) or np.any((w[1:] >= 2048) & (w[:-1] <= 1))
    assert len(rg["rid"]) == nb + len(deck.ISLAND_COUNTS) + len(deck.LONG_COUNTS) + 2 * len(deck.C0_COUNTS)
    # every island has its range [1024, 3072), in the deck and among the sums' ranges
    for ranges in (rg, deck.sum_ranges()):
        isl = slice(len(ranges["rid"]) - len(deck.island_refs()), None)
        assert np.array_equal(ranges["rid"][isl], deck.island_refs())
        assert np.all(ranges["loc"][isl] == deck.ISLAND_LO) and np.all(ranges["len"][isl] == deck.ISLAND_HI - deck.ISLAND_LO)


def test_cuts_leave_the_residues():
    for tile in deck.TILES + (None,):
        seen = set()
        for residue in (0, 7, 1):
            rg, k = deck.cut(tile, residue)
            assert int(deck.tiles_of(rg, tile).sum()) % 8 == residue
            assert len(rg["len"]) == len(deck.ranges()["len"]) - k
            assert deck.cut_expected("half_ss0", k).size == int(rg["len"].sum())
            seen.add(k)
        assert len(seen) == 3


def test_every_parameter_set_counts_something_within_16_bits():
    for name, (entry, args) in deck.PARAM_SETS.items():
        want, off = deck.expected(name)
        assert want.dtype == np.int32 and want.any(), name
        assert len(off) == len(deck.ranges()["len"]) + 1 and off[-1] == want.size
        if args["binsize"] == 1:                                 # the per-base images: 16-bit cells
            assert 0 <= want.min() and want.max() <= 32_767, (name, int(want.max()))
        # an island's range counts the island's reads whose 5' end lies in it, whatever the bins and strands
        if entry == "pileup" and args.get("shift", 0) == 0:
            c = deck.reads()
            five = np.where((c["flag"] & 16) != 0, c["end"], c["pos"])
            inside = (five >= deck.ISLAND_LO) & (five < deck.ISLAND_HI)
            for i, r in enumerate(deck.island_refs()):
                seg = want[off[deck.N_BULK_RANGES + i]:off[deck.N_BULK_RANGES + i + 1]]
                assert seg.sum() == inside[c["ref_off"][r]:c["ref_off"][r + 1]].sum(), (name, i)
    for name in deck.SUM_SETS:
        s = deck.expected_sum(name)
        assert s.dtype == np.int64 and s.any(), name


# ---------------------------------------------------------------------------------------------------------------
# the later forms (tests/test_later_forms_gpu.py, whose case tables are read here): conditions on the input, so that no
# GPU case is vacuous
# ---------------------------------------------------------------------------------------------------------------
def _capped_cell_sets():
    """the (shift, mapqual) of every capped case: a word form on a packed layout comes from mapqual 10"""
    import test_later_forms_gpu as lf
    return sorted({(c[6], 10 if c[1] else 0) for c in lf.CAPPED})


def test_capped_cells_lie_on_both_sides_of_every_cap():
    import test_later_forms_gpu as lf
    assert _capped_cell_sets() == [(0, 0), (0, 10), (75, 0), (75, 10)]
    n_ranges = len(deck.ranges()["len"])
    for shift, mapqual in _capped_cell_sets():
        cells = deck.capped_cells(shift, mapqual)
        assert len(cells) == n_ranges and all(c.dtype == np.int64 and c.shape == (2, w) for c, w in zip(cells, deck.ranges()["len"]))
        for row in (0, 1):
            v = np.concatenate([c[row] for c in cells])
            for k in lf.CAPPED_KS:
                assert (v > k).any() and ((v >= 1) & (v <= k)).any(), (shift, mapqual, row, k)
            assert v.max() <= 11                                 # (a cap of 11 would bite nowhere: the claim can fail)
    # the island ranges without a filter or a shift: cells up to 11, most of the non-zero ones 1, some above every cap
    isl = np.concatenate([c.reshape(-1) for c in deck.capped_cells(0, 0)[deck.N_BULK_RANGES:]])
    assert (int(isl.max()), int((isl == 1).sum()), int((isl > 5).sum())) == (11, 64_104, 781)
    # a coverage case's mapqual filter and cap too
    for c in lf.CAPPED_COVER:
        want, off = deck.expected_capped_cover(c[6], c[2], c[3], c[4], 10 if c[1] else 0)
        assert want.dtype == np.int64 and want.any() and off[-1] == want.size, c
        if c[2] == 1 and c[3] == 1:                              # a fragment of one base: the capped cells themselves
            flat = deck.expected_capped(c[6], 1, c[4], 0, 10 if c[1] else 0)[0]
            assert np.array_equal(want, flat) and c[6] <= want.max() <= (1 if c[4] else 2) * c[6], c


def add_classes(cells, tile_cells, binsize, ss):
    """Which branches of CappedCells::add (csrc/kernels.hip) the deck's ranges reach, restated: a range of w per-base cells
    is cut into tiles of tile_cells (rounded up to whole fours), a wave walks the cells [64 j, 64 j + 64) of a tile -- the
    lanes behind the tile's last cell hold nothing --, and what it adds is the sense row, then the antisense row (with
    strands) or their sum (without).  A stretch with
      a: 1 .. 16 non-zero cells lets them add for themselves;
      b: more, every lane a cell and all in one bin, takes the xor reduction;
      c: more, every lane a cell, in two or more bins, takes the segmented scan;
      d: more, in a tile's last, partial stretch (the lanes behind it differ from every bin), takes the scan too.
    A capped cell is zero exactly where the uncapped one is."""
    tile = (tile_cells + 3) & ~3
    met = set()
    for c in cells:
        w = c.shape[1]
        rows = (c[0], c[1]) if ss else (c[0] + c[1],)
        for c0 in range(0, w, tile):
            nc = min(tile, w - c0)
            for j in range(0, nc, 64):
                n = min(64, nc - j)
                first, last = ((c0 + j) // binsize, (c0 + j + n - 1) // binsize) if binsize > 0 else (0, 0)
                for r in rows:
                    nz = int(np.count_nonzero(r[c0 + j:c0 + j + n]))
                    if nz:
                        met.add("a" if nz <= 16 else "d" if n < 64 else "b" if first == last else "c")
    return met


def test_capped_cases_reach_every_branch_of_add():
    import test_later_forms_gpu as lf
    shapes = sorted({(c[4], c[2], c[3], c[6], 10 if c[1] else 0) for c in lf.CAPPED if c[2] != 1})
    assert {(t, b) for t, b, _, _, _ in shapes} == {(t, b) for t in lf.CAPPED_TILES for b in (7, 274, -1)}
    union = {False: set(), True: set()}
    for tile, binsize, ss, shift, mapqual in shapes:
        met = add_classes(deck.capped_cells(shift, mapqual), tile, binsize, ss)
        union[ss] |= met
        what = (tile, binsize, ss, shift, mapqual, sorted(met))
        assert "a" in met, what
        if tile == 16:                       # at most 16 cells a stretch: nothing but the lanes' own adds
            assert met == {"a"}, what
        elif tile == 18:                     # 20 cells, one partial stretch a tile: the densest islands fill more than 16
            assert met == {"a", "d"}, what
        elif binsize < 0:                    # bamCount: one bin
            assert "b" in met and "c" not in met, what
        elif binsize == 274:                 # a bin of at least a tile: a stretch lies in one or straddles two
            assert {"b", "c"} <= met, what
        else:                                # bins of 7: nine or ten a stretch
            assert "c" in met and "b" not in met, what
    assert union[False] == union[True] == set("abcd")
    # (the aligned 64-cell stretches of the island ranges, strands apart: both sides of the 16 non-zero lanes)
    nz = np.concatenate([np.count_nonzero(c.reshape(2, -1, 64), axis=2).reshape(-1) for c in deck.capped_cells(0, 0)[deck.N_BULK_RANGES:]])
    assert (int(((nz >= 1) & (nz <= 16)).sum()), int((nz > 16).sum())) == (3842, 2222)
    # a bin size that leaves a class empty is seen
    assert "c" not in add_classes(deck.capped_cells(0, 0), 256, 8192, False)


def test_capped_coverage_rows_straddle_the_scans_rounds():
    """k_capped_scan carries from one round of 256 pairs to the next: rows of 256 k - 1, 256 k and 256 k + 1 pairs for the
    first round's end and the eighth's, among the scratch rows of the capped coverage cases"""
    import test_later_forms_gpu as lf
    lengths = {c[2] for c in lf.CAPPED_COVER}
    rows = np.concatenate([deck.capped_cover_rows(L) for L in lengths])
    for n in (255, 256, 257, 2047, 2048, 2049):
        assert (rows == n).any(), n
    rg = deck.ranges()
    # a fragment of one base widens nothing: a row is its range, less the bases of the ranges that begin at -3
    assert np.array_equal(deck.capped_cover_rows(1), np.where(rg["len"] > 0, rg["len"] + np.minimum(rg["loc"], 0), 0))
    assert int(np.sum(rg["loc"] < 0)) == 3
    # widened by L - 1 on both sides, less what lies below base 0
    w36 = deck.capped_cover_rows(36)
    assert np.all(w36[rg["len"] > 0] <= rg["len"][rg["len"] > 0] + 70) and np.any(w36[rg["len"] > 0] < rg["len"][rg["len"] > 0] + 70)
    assert not w36[rg["len"] == 0].any()


def test_vplot_shapes_count_both_island_groups_and_their_edges():
    import test_later_forms_gpu as lf
    srg = deck.sum_ranges()
    assert len(srg["len"]) == 198 and set(srg["len"].tolist()) == {deck.SUM_WIDTH} and set(srg["strand"].tolist()) == {1, -1, 0}
    assert deck.VPLOT_CELLS == {"small": 3526, "budget": 40_960, "below": 38_912, "above": 43_008}
    shapes = {(lf.VPLOT_WHICH[c[1]][0], c[3], c[6]) for c in lf.VPLOT}
    assert {s for s, _, _ in shapes} == set(deck.VPLOT_SHAPES)
    for shape, midpoint, mapqual in sorted(shapes):
        tf, len_bin, binsize = deck.VPLOT_SHAPES[shape]
        assert tf[1] <= 600
        whole = deck.expected_vplot(tf, len_bin, binsize, midpoint, mapqual)
        assert whole.dtype == np.int64 and whole.shape == (tf[1] // len_bin + 1, -(-deck.SUM_WIDTH // binsize))
        assert whole.size == deck.VPLOT_CELLS[shape]
        assert whole.max() >= 2 and whole[:, 0].any() and whole[:, -1].any(), (shape, midpoint, mapqual)
        assert not whole[:tf[0] // len_bin].any()
        for which in ("c0", "paired"):
            part = deck.expected_vplot(tf, len_bin, binsize, midpoint, mapqual, which)
            assert part.any() and np.all(part <= whole), (shape, midpoint, mapqual, which)
    # the budget shapes are one table of exactly 160 KiB of 32-bit counters, one row fewer and one row more
    assert 4 * deck.VPLOT_CELLS["budget"] == 160 * 1024
    assert deck.VPLOT_CELLS["budget"] - deck.VPLOT_CELLS["below"] == deck.VPLOT_CELLS["above"] - deck.VPLOT_CELLS["budget"] == 2048
    # the small shape under 14 KiB: the counters fit, the filter table's 512 bytes behind them do not
    assert 4 * deck.VPLOT_CELLS["small"] <= 14 * 1024 < 4 * ((deck.VPLOT_CELLS["small"] + 3) & ~3) + 512
    # the mapqual filter of the word-form case drops something
    small = deck.VPLOT_SHAPES["small"]
    assert deck.expected_vplot(*small, True, 10).sum() < deck.expected_vplot(*small, True).sum()


def test_resized_sets_count_something_within_16_bits():
    import test_later_forms_gpu as lf
    psets = {"cover", "bins2_ss0", "bins2_ss1"} | {p for p, _, _, _ in lf.COV_BINS}
    for L in lf.RESIZED_L:
        for pset in sorted(psets):
            want, off = deck.expected_resized(L, pset)
            assert want.dtype == np.int32 and want.any() and off[-1] == want.size, (L, pset)
        # per base: the tile images' signed 16-bit cells hold it without the heavy-tile knob
        cover = deck.expected_resized(L, "cover")[0]
        assert 0 <= cover.min() and cover.max() <= 32_767, (L, int(cover.max()))
        for ss in (False, True):
            s = deck.expected_resized_sum(L, ss)
            assert s.dtype == np.int64 and s.any() and s.size == deck.SUM_WIDTH * (2 if ss else 1)
        assert deck.expected_resized_sum(L, False).sum() == deck.expected_resized_sum(L, True).sum()
    # a longer fragment covers more
    assert deck.expected_resized(36, "cover")[0].sum() < deck.expected_resized(5000, "cover")[0].sum()
