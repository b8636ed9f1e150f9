"""The claims of tests/forms_deck.py about its own reads and ranges, checked with the C oracle alone: the islands hold the
counts they name, their windows start at every residue modulo 8 in every class they are there for, the ranges meet every
value of out_off & 3 at every width, the cuts leave the tile counts they promise, every parameter set of the matrix
counts something, and no cell leaves the 16-bit tile images' range without the heavy-tile knob."""
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
    isl = slice(int(c["ref_off"][len(deck.BULK_REFS)]), None)
    assert c["pos"][isl].min() >= deck.ISLAND_LO and c["pos"][isl].max() < deck.ISLAND_HI
    assert set(c["flag"][isl].tolist()) == {0, 16} and set(c["mapq"][isl].tolist()) == {deck.ISLAND_MAPQ}
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
                                    (False, 1, c["long_refs"], c["long_m"]), (False, 2, c["long_refs"], c["long_m"])):
        start, count = deck.island_windows(packed, cls_id, refs)
        assert np.array_equal(count, m), (packed, cls_id)                      # nj == m: all of them in the one class
        assert set((start[m > 0] % 8).tolist()) == set(range(8)), (packed, cls_id)
    # the default layout packs every short island read and leaves some of the bulk's short reads in class 0
    cls = deck.read_classes(True)
    span = c["end"].astype(np.int64) - c["pos"] + 1
    assert np.any((cls == 0) & (span <= 256)) and np.any(cls == 3)
    assert not np.any(deck.read_classes(False) == 4)


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
    assert len(rg["rid"]) == nb + len(deck.ISLAND_COUNTS) + len(deck.LONG_COUNTS)


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
            for i, r in enumerate(np.concatenate([c["short_refs"], c["long_refs"]])):
                seg = want[off[deck.N_BULK_RANGES + i]:off[deck.N_BULK_RANGES + i + 1]]
                assert seg.sum() == inside[c["ref_off"][r]:c["ref_off"][r + 1]].sum(), (name, i)
    for name in deck.SUM_SETS:
        s = deck.expected_sum(name)
        assert s.dtype == np.int64 and s.any(), name
