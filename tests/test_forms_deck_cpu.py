"""The claims of tests/forms_deck.py about its own reads and ranges, checked with the C oracle alone: the islands hold the
counts they name, their windows start at every residue modulo 8 in every class they are there for (the class-0 islands in
class 0 of both layouts, the paired islands in the packed class), the ranges meet every
value of out_off & 3 at every width, the cuts leave the tile counts they promise, every parameter set of the matrix
counts something, and no cell leaves the 16-bit tile images' range without the heavy-tile knob."""
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
