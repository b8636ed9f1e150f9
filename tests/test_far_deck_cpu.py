"""The claims of tests/far_deck.py and of the expected sides tests/test_far_genome_gpu.py compares with, checked without a
GPU: where every placement puts the decks (the numbers written out), that no int arithmetic of the C oracle and no refusal
of the library is approached, that the expected side computed directly at a far placement is the near one moved by D
(translation invariance: a theorem for every range that does not hang below base 0, so a difference would be an overflow
in the oracle or in a restatement), and that no case is vacuous -- the cells hold counts, and behind 2^32 a read whose
coordinate lost bit 32 would be looked for in an empty spacer."""
import itertools

import numpy as np
import pytest

import far_deck as fd
import forms_deck as deck
import genecounts_expected as gx
import junctions_expected as jx
import spliced_expected as sx
import test_far_genome_gpu as far_gpu

I32_MAX = 2 ** 31 - 1
FILTERS = far_gpu.FILTERS

# the forms deck: the cumulative first unit (64 kbp) of the three bulk references and of the first island, and the
# genome's total, per placement -- cumulative base = unit << 16, so 65,536 is 2^32 and 1,048,576 is 2^36
FORMS_UNITS = {
    "past_2_32": ([65_536, 65_538, 65_540, 65_542], 65_680),
    "straddle_2_32": ([65_533, 65_535, 65_537, 65_539], 65_677),
    "past_2_36": ([1_048_576, 1_048_578, 1_048_580, 1_048_582], 1_048_720),
    "deep_2_30": ([0, 16_385, 32_770, 49_155], 2_310_147),
    "top": ([98_304, 131_071, 163_838, 196_605], 4_718_313),
}
FORMS_TOP_D = 2_147_344_754                     # 2^31 - 1 - 1,000 - 137,893 (the deck's largest read end)
# units in front of a deck's first reference, whatever the deck
FRONT_UNITS = {"past_2_32": 65_536, "straddle_2_32": 65_533, "past_2_36": 1_048_576, "deep_2_30": 0, "top": 98_304,
               "k1": 32_768, "k2": 65_536, "k5": 163_840, "k6": 196_608, "k29": 950_272, "k30": 983_040}
ALL_DECKS = ("hand", "random", "junction", "genes_hand", "genes_random")


# ---------------------------------------------------------------------------------------------------------------
# the placements' claims
# ---------------------------------------------------------------------------------------------------------------
def test_spacer_and_filler_units():
    assert fd.units([fd.SPACER_LEN])[0] == fd.SPACER_UNITS == 32_768 and fd.SPACER_LEN == I32_MAX
    assert fd.units([fd.filler_len(32_765)])[0] == 32_765
    assert set(fd.FIVE) == set(FORMS_UNITS) and set(fd.ELEVEN) == set(FRONT_UNITS) and len(fd.ELEVEN) == 11
    assert fd.NAMED["deep_2_30"][1] == 2 ** 30 - 35_000 and fd.NAMED["deep_2_30"][1] % 32_768 != 0


@pytest.mark.parametrize("name", fd.FIVE)
def test_forms_deck_lies_where_the_table_says(name):
    p = deck.named_placement(name)
    c, near = deck.reads(p), deck.reads()
    front = fd.refs_in_front(p)
    u0 = fd.unit0(c["ref_len"])
    want, total = FORMS_UNITS[name]
    assert u0[front:front + 4].tolist() == want and u0[front] == FRONT_UNITS[name] and int(u0[-1]) == total < 2 ** 31
    assert len(c["ref_len"]) == len(near["ref_len"]) + front and np.all(np.diff(c["ref_off"][:front + 1]) == 0)
    assert np.array_equal(np.diff(c["ref_off"][front:]), np.diff(near["ref_off"]))
    g = fd.cumulative(c)
    if name == "past_2_32":
        assert int(u0[front]) << 16 == 2 ** 32 and g.min() >= 2 ** 32
    if name == "straddle_2_32":
        # the second bulk reference (65,536 bases) takes units 65,535 and 65,536: its reads start below 2^32 and hundreds
        # of them end behind it, ranges hang over its last base into the unit at 2^32, and everything behind lies past 2^32
        a, b = int(c["ref_off"][front + 1]), int(c["ref_off"][front + 2])
        g_end = g + (c["end"].astype(np.int64) - c["pos"])
        assert g[:b].max() < 2 ** 32 and g[b:].min() >= 2 ** 32 + 65_536 and np.count_nonzero(g_end[a:b] >= 2 ** 32) > 500
        rg = deck.ranges(p)
        on = rg["rid"] == front + 1
        assert np.any(on & (rg["loc"] < 65_536) & (rg["loc"].astype(np.int64) + rg["len"] > 65_536))
    if name == "past_2_36":
        assert int(u0[front]) << 16 == 2 ** 36 and len(c["ref_len"]) == len(near["ref_len"]) + 32
    if name == "deep_2_30":
        assert p.D == 1_073_706_824 and p.D % 65_536 != 0 and p.D % 32_768 != 0
        for r in range(3):                  # the bulk references' reads lie on both sides of base 2^30 of their reference
            q = c["pos"][int(c["ref_off"][r]):int(c["ref_off"][r + 1])]
            assert np.any(q < 2 ** 30) and np.any(q >= 2 ** 30)
    if name == "top":
        assert p.D == FORMS_TOP_D and int(c["end"].max()) == I32_MAX - fd.TOP_HEADROOM and g.min() >= 2 ** 32
    # the move itself: every column but pos and end is the deck's own
    assert np.array_equal(c["pos"].astype(np.int64) - p.D, near["pos"]) and np.array_equal(c["end"].astype(np.int64) - p.D, near["end"])
    assert np.array_equal(c["ref_len"][front:].astype(np.int64) - p.D, near["ref_len"])
    for k in ("flag", "mapq", "tlen"):
        assert c[k] is near[k]
    for table in (deck.ranges, deck.sum_ranges):
        rg, rg0 = table(p), table()
        assert np.array_equal(rg["rid"], rg0["rid"] + front) and np.array_equal(rg["loc"].astype(np.int64) - p.D, rg0["loc"])
        assert rg["len"] is rg0["len"] and rg["strand"] is rg0["strand"]
        back = fd.unplace_ranges(rg, p)
        assert np.array_equal(back["rid"], rg0["rid"]) and np.array_equal(back["loc"], rg0["loc"])


@pytest.mark.parametrize("name", fd.ELEVEN)
@pytest.mark.parametrize("which", ALL_DECKS)
def test_spliced_decks_lie_where_the_table_says(which, name):
    near, far = fd.near(which), fd.far(which, name)
    p, c = far.placement, far.cols
    front = fd.refs_in_front(p)
    u0 = fd.unit0(c["ref_len"])
    assert int(u0[front]) == FRONT_UNITS[name] and int(u0[-1]) < 2 ** 31
    assert front == {"straddle_2_32": 2, "past_2_32": 2, "past_2_36": 32, "deep_2_30": 0, "top": 3}.get(name, p.K)
    assert np.array_equal(c["pos"].astype(np.int64) - p.D, near.cols["pos"]) and c["cigar"] is not near.cols["cigar"]
    assert np.array_equal(c["cigar"], near.cols["cigar"]) and c["cigar_off"] is near.cols["cigar_off"]
    assert np.array_equal(c["end"].astype(np.int64) - p.D, near.cols["end"])             # end moves with pos: CIGARs unchanged
    if which != "genes_random":                 # (that deck makes reads unmapped in a copy and keeps the mapped reads' ends)
        assert np.array_equal(sx.ends(c), c["end"])
    if name in fd.K_ONLY and len(near.cols["ref_len"]) == 3:
        # three references behind K spacers: n_ref = 2^k with the last reference's id 2^k - 1, or one more
        n_ref = len(c["ref_len"])
        assert n_ref == 3 + p.K and n_ref in (4, 5, 8, 9, 32, 33)
        assert int(np.flatnonzero(np.diff(c["ref_off"]) > 0)[-1]) == n_ref - 1 and (n_ref - 1) in (3, 4, 7, 8, 31, 32)
    if name == "top":
        ranged = list(near.tables.values()) + ([near.ann.features] if near.ann is not None else [])
        ends = [int((fd.place_ranges(t, p)["loc"].astype(np.int64) + t["len"]).max()) for t in ranged]
        assert max([int(c["end"].max()), int(c["ref_len"][front:].max())] + ends) == I32_MAX - fd.TOP_HEADROOM
    if name in ("past_2_32", "past_2_36", "top"):
        assert fd.cumulative(c).min() >= 2 ** 32 - 65_536       # (a read of the hand deck starts at base -1)


# ---------------------------------------------------------------------------------------------------------------
# headroom: what the oracle forms in int, and what the library refuses
# ---------------------------------------------------------------------------------------------------------------
def test_oracle_int_arithmetic_keeps_its_headroom_on_the_forms_deck():
    """oracle/bamsignals_oracle.c forms loc + len (ga_end), end + 1 - loc, pos + |tlen| / 2 + shift (the 5' end) and, for
    tspan, pos + tlen - 1 in int; the resized and the capped coverage's restatements add frag_len.  With every parameter
    set the far module runs these stay below 2^31 at every placement: `top` stops 1,000 bases short for this."""
    reach = far_gpu.parameter_reach()
    assert reach == {"shift": 75, "tlen": 600, "frag_len": 36} and max(reach.values()) < fd.TOP_HEADROOM
    assert reach["shift"] + reach["tlen"] // 2 < fd.TOP_HEADROOM           # midpoint: 5' end + shift + tlen / 2
    for name in fd.FIVE:
        p = deck.named_placement(name)
        c = deck.reads(p)
        for rg in (deck.ranges(p), deck.sum_ranges(p)):
            assert int((rg["loc"].astype(np.int64) + rg["len"]).max()) + reach["tlen"] + reach["shift"] < 2 ** 31
        top = max(int(c["end"].max()) + 1, int(c["pos"].max()))
        assert top + reach["shift"] + reach["tlen"] // 2 < 2 ** 31 and top + reach["tlen"] < 2 ** 31 and top + reach["frag_len"] < 2 ** 31
        assert int(c["pos"].min()) - reach["tlen"] - reach["shift"] > -2 ** 31


def test_no_library_refusal_is_approached():
    """a feature must end at or below base 2^31 - 1 (csrc/genemodel.h), shift / tlen filter stay at or below 2^30
    (bsig_plan_create), a reference has at most 2^31 - 1 bases and the genome fewer than 2^31 units"""
    reach = far_gpu.parameter_reach()
    assert reach["shift"] + reach["tlen"] <= 2 ** 30
    for which, name in itertools.product(ALL_DECKS, fd.ELEVEN):
        near, far = fd.near(which), fd.far(which, name)
        assert int(far.cols["ref_len"].max()) <= I32_MAX and int(fd.unit0(far.cols["ref_len"])[-1]) < 2 ** 31
        for t in list(far.tables.values()) + ([far.features] if far.features is not None else []):
            assert int((t["loc"].astype(np.int64) + t["len"]).max()) <= I32_MAX - fd.TOP_HEADROOM
        assert len(near.cols["pos"]) == len(far.cols["pos"]) > 0


# ---------------------------------------------------------------------------------------------------------------
# translation invariance on the forms deck
# ---------------------------------------------------------------------------------------------------------------
def _hanging(rg):
    """the ranges that hang below base 0 of their reference where the deck is: the bases in front of them exist once the
    deck is moved by D > 0"""
    return np.flatnonzero(rg["loc"] < 0)


def test_the_ranges_that_hang_below_base_zero():
    assert _hanging(deck.ranges()).tolist() == far_gpu.HANGING_RANGES and np.all(deck.ranges()["loc"][far_gpu.HANGING_RANGES] == -3)
    assert _hanging(deck.sum_ranges()).tolist() == far_gpu.HANGING_SUM_RANGES == [0] and deck.sum_ranges()["loc"][0] == -5


@pytest.mark.parametrize("name", fd.FIVE)
def test_forms_per_range_sets_do_not_depend_on_the_placement(name):
    """Every per-range parameter set, range by range.  The hanging ranges are compared too and turn out equal: the oracle
    does not cut a range at base 0 (rel = pos5 - loc; a - (loc) for coverage), and no read of the deck starts below its
    reference's base 0, so the bases in front of the deck's references hold nothing at any placement either."""
    p = deck.named_placement(name)
    hang = set(far_gpu.HANGING_RANGES)
    differ = {}
    for pset in deck.PARAM_SETS:
        (near, off0), (far, off) = deck.expected(pset), deck.expected(pset, p)
        assert np.array_equal(off, off0) and far.dtype == near.dtype == np.int32
        bad = [i for i in range(len(off) - 1) if not np.array_equal(far[off[i]:off[i + 1]], near[off0[i]:off0[i + 1]])]
        assert not set(bad) - hang, (pset, bad[:8])                 # a theorem: an overflow in the oracle or a helper
        if bad:
            differ[pset] = bad
        assert far.max() > 0, pset
    assert differ == {}, "the hanging ranges that differ, by index"


@pytest.mark.parametrize("name", fd.FIVE)
def test_forms_sums_and_later_kinds_do_not_depend_on_the_placement(name):
    """The reductions have no per-range side to leave the hanging ranges out of; none of those differs (above), so every
    reduction is compared whole.  The later kinds' sets are the far module's own."""
    p = deck.named_placement(name)
    for sset in deck.SUM_SETS:
        far = deck.expected_sum(sset, p)
        assert np.array_equal(far, deck.expected_sum(sset)) and far.max() > 0, sset
    seen = set()
    for kind, near, far in far_gpu.later_expected_pairs(p):
        for a, b in zip(near if isinstance(near, tuple) else (near,), far if isinstance(far, tuple) else (far,)):
            assert np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b), kind
        first = far[0] if isinstance(far, tuple) else far
        assert np.asarray(first).max() > 0, kind
        seen.add(kind)
    assert seen == set(far_gpu.LATER_KINDS)


@pytest.mark.parametrize("name", ["past_2_32", "past_2_36", "top"])
def test_behind_2_32_a_lost_bit_lands_in_a_spacer(name):
    """g mod 2^32 of every read lies in a spacer, which holds no read: a kernel that dropped bit 32 would find nothing"""
    for c in [deck.reads(deck.named_placement(name))] + [fd.far(which, name).cols for which in ALL_DECKS]:
        K = fd.NAMED[name][0]
        g = fd.cumulative(c)
        alias = fd.aliased_reference(c, g % 2 ** 32)
        assert np.all((alias >= 0) & (alias < K)) and np.all(np.diff(c["ref_off"][:K + 1]) == 0)


# ---------------------------------------------------------------------------------------------------------------
# translation invariance on the spliced, junction and gene-count decks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fd.ELEVEN)
@pytest.mark.parametrize("which", fd.SPLICED_DECKS)
def test_spliced_expected_sides_do_not_depend_on_the_placement(which, name):
    near, far = fd.near(which), fd.far(which, name)
    p = far.placement
    b0, b = fd.blocks(which), fd.blocks(which, name)
    assert np.array_equal(b["pos"].astype(np.int64) - p.D, b0["pos"]) and np.array_equal(b["end"].astype(np.int64) - p.D, b0["end"])
    assert np.array_equal(b["read"], b0["read"]) and np.array_equal(b["ref_off"][fd.refs_in_front(p):], b0["ref_off"])
    for binsize, ss, flt in far_gpu.COVERAGE_SETS:
        want = sx.expected_coverage(b, far.tables["tiles"], binsize=binsize, ss=ss, **flt)
        assert np.array_equal(want, sx.expected_coverage(b0, near.tables["tiles"], binsize=binsize, ss=ss, **flt)) and want.max() > 0
    jr0, jr = fd.junction_rows(which), fd.junction_rows(which, name)
    back = fd.unplace_rows(jr, p)
    for k in jr0:
        assert np.array_equal(back[k], jr0[k]), k
    total = 0
    sets = list(itertools.product((False, True), FILTERS, far_gpu.ANCHORS))
    if name in fd.K_ONLY:                       # (only the reference ids move: the two corners of the product)
        sets = [sets[0], sets[-1]]
    for table, (ss, flt, anchor) in itertools.product(far_gpu.JUNCTION_TABLES, sets):
        want = jx.expected(jr, far.tables[table], ss=ss, min_anchor=anchor, **flt)
        assert jx.same(fd.unplace_junctions(want, p), jx.expected(jr0, near.tables[table], ss=ss, min_anchor=anchor, **flt))
        total += int(want[0][-1])
        assert want[0][-1] > 0 or which == "hand", (table, ss, flt, anchor)
    assert total > 0


@pytest.mark.parametrize("name", fd.ELEVEN)
@pytest.mark.parametrize("which", list(fd.GENE_DECKS))
def test_gene_count_expected_sides_do_not_depend_on_the_placement(which, name):
    near, far = fd.near(which), fd.far(which, name)
    ann = near.ann
    for mode, flt in itertools.product(gx.MODES, FILTERS):
        counts, summary = gx.expected(far.cols, far.features, ann.gene, ann.n_genes, strand=mode, **flt)
        counts0, summary0 = gx.expected(near.cols, ann.features, ann.gene, ann.n_genes, strand=mode, **flt)
        assert np.array_equal(counts, counts0) and np.array_equal(summary, summary0), (mode, flt)
        assert summary[0] > 0 and counts.max() > 0 and summary.sum() == len(near.cols["pos"])
