"""Placements: a deck's reads, ranges and features moved to far genome coordinates (a helper, not a conftest).

The resident layout addresses a read by the cumulative coordinate ``g = (ref_unit0 << 16) + pos``: references back to back,
each rounded up to ``(ref_len >> 16) + 1`` units of 64 kbp (csrc/runtime.hip: layout_from_device).  The decks of the suite
live below cumulative 2^24; a placement ``(K, D, filler)`` moves one where 32-bit arithmetic would slip:

  * ``K`` empty spacer references of 2^31 - 1 bases (32,768 units, 2^31 cumulative bases each) stand in front of the deck's
    references -- behind them, where ``filler`` is not 0, one more empty reference of exactly ``filler`` units;
  * ``D`` bases are added to every position of every deck reference, and every deck reference grows by ``D``: a read keeps
    its relation to its reference's last base.  CIGARs stay as they are, ``end`` moves with ``pos``.

A range or a feature moves by ``D``, its ``rid`` by the number of references put in front.  Spacers and filler hold no reads.
What a result states relative to its range (cells, runs, views, summits, counts) does not move; what it states in reference
coordinates (a junction's start and end) moves by ``D``: ``unplace_junctions`` takes it back.

Everything is computed in int64 and checked against int32 before it is cast: a placement that does not fit is an error here,
never a wrapped column."""
from __future__ import annotations

import collections
import functools

import numpy as np

I32_MAX = 2 ** 31 - 1
UNIT_SHIFT = 16                                 # BSIG_REF_UNIT_SHIFT
SPACER_LEN = I32_MAX                            # the longest reference the library takes
SPACER_UNITS = 32_768
TOP_HEADROOM = 1_000                            # bases `top` leaves below 2^31 - 1 for shift, template length and frag_len

Placement = collections.namedtuple("Placement", "name K D filler")

# name -> (K, D, filler units); D None: computed from the deck (top_shift)
NAMED = {
    "past_2_32": (2, 0, 0),                     # the deck's first reference begins at cumulative 2^32 exactly
    "straddle_2_32": (1, 0, 32_765),            # the deck's references take units 65,533 on: the second crosses 2^32
    "past_2_36": (32, 0, 0),                    # cumulative 2^36
    "deep_2_30": (0, 2 ** 30 - 35_000, 0),      # base 2^30 lies 35,000 bases into every reference that is long enough
    "top": (3, None, 0),                        # both: the deck's last base as close to 2^31 - 1 as the headroom allows
}
FIVE = tuple(NAMED)
# the spliced decks: n_ref = 2^k and 2^k + 1 for decks of three references (the radix sorts' 32 + ref_bits key range)
K_ONLY = tuple(f"k{K}" for K in (1, 2, 5, 6, 29, 30))
NAMED.update({f"k{K}": (K, 0, 0) for K in (1, 2, 5, 6, 29, 30)})
ELEVEN = FIVE + K_ONLY


def units(ref_len):
    """64-kbp units per reference, as layout_from_device counts them"""
    return (np.asarray(ref_len, np.int64) >> UNIT_SHIFT) + 1


def unit0(ref_len):
    """the cumulative first unit of every reference, and the total behind them (n_ref + 1 values)"""
    return np.concatenate([[0], np.cumsum(units(ref_len))])


def filler_len(filler_units):
    """a reference length that takes exactly `filler_units` units (the shortest one)"""
    return (int(filler_units) - 1) << UNIT_SHIFT


def top_shift(cols, *ranged):
    """D of `top`: the largest shift that leaves TOP_HEADROOM bases between 2^31 - 1 and the largest of: a reference's
    length, a read's ``end`` (reads may hang past their reference's end), and ``loc + len`` of any of the ranges or features
    `ranged` (dicts with loc and len; that is one past a feature's last base)"""
    top = int(np.asarray(cols["ref_len"], np.int64).max(initial=0))
    if len(cols["pos"]):
        top = max(top, int(np.asarray(cols["end"], np.int64).max()), int(np.asarray(cols["pos"], np.int64).max()))
    for rg in ranged:
        if len(rg["loc"]):
            top = max(top, int((np.asarray(rg["loc"], np.int64) + np.asarray(rg["len"], np.int64)).max()))
    return I32_MAX - TOP_HEADROOM - top


def placement(name, cols=None, *ranged):
    """the named placement; `top` needs the deck's columns and whatever ranges and features will be placed with them"""
    K, D, filler = NAMED[name]
    if D is None:
        D = top_shift(cols, *ranged)
    return Placement(name, K, int(D), filler)


def refs_in_front(p):
    return p.K + (1 if p.filler else 0)


def _i32(a, what):
    a = np.asarray(a, np.int64)
    assert a.min(initial=0) >= -2 ** 31 and a.max(initial=0) <= I32_MAX, f"{what} leaves int32 at this placement"
    return a.astype(np.int32)


def place_columns(cols, p):
    """Plain or CIGAR columns at placement `p`: ref_len, ref_off, pos and end (where there is one) move, every other column is
    the deck's own -- except ``cigar``, which is copied, because genecounts_expected keeps a read's blocks by that array's
    identity.  Keys that end in ``_refs`` (forms_deck: the islands' reference ids) move with the references."""
    front = refs_in_front(p)
    head = [SPACER_LEN] * p.K + ([filler_len(p.filler)] if p.filler else [])
    out = dict(cols)
    out["ref_len"] = _i32(np.concatenate([np.asarray(head, np.int64), np.asarray(cols["ref_len"], np.int64) + p.D]), "ref_len")
    out["ref_off"] = np.concatenate([np.zeros(front, np.int64), np.asarray(cols["ref_off"], np.int64)])
    out["pos"] = _i32(np.asarray(cols["pos"], np.int64) + p.D, "pos")
    if "end" in cols:
        out["end"] = _i32(np.asarray(cols["end"], np.int64) + p.D, "end")
    if "cigar" in cols:
        out["cigar"] = np.array(cols["cigar"], copy=True)
    for k, v in cols.items():
        if k.endswith("_refs"):
            out[k] = np.asarray(v) + front
    for k in ("ref_len", "ref_off", "pos", "end", "cigar"):
        if k in out:
            out[k].setflags(write=False)
    return out


def place_ranges(rg, p):
    """ranges (rid, loc, len, strand) at placement `p`; loc + len must stay in int32, as every consumer forms it"""
    out = dict(rg)
    out["rid"] = _i32(np.asarray(rg["rid"], np.int64) + refs_in_front(p), "rid")
    out["loc"] = _i32(np.asarray(rg["loc"], np.int64) + p.D, "loc")
    _i32(np.asarray(out["loc"], np.int64) + np.asarray(rg["len"], np.int64), "loc + len")
    for k in ("rid", "loc"):
        out[k].setflags(write=False)
    return out


place_features = place_ranges                   # a feature table has a range table's columns


def unplace_ranges(rg, p):
    out = dict(rg)
    out["rid"] = (np.asarray(rg["rid"], np.int64) - refs_in_front(p)).astype(np.int32)
    out["loc"] = (np.asarray(rg["loc"], np.int64) - p.D).astype(np.int32)
    return out


def unplace_junctions(result, p):
    """a junction result (seg_off, start, end, count, max_anchor) with start and end taken back by D"""
    seg_off, start, end, count, anchor = result
    return seg_off, np.asarray(start, np.int64) - p.D, np.asarray(end, np.int64) - p.D, count, anchor


def unplace_rows(jr, p):
    """junction rows (junctions_expected.rows) taken back to the near deck: ref, ref_off, start and end"""
    front = refs_in_front(p)
    out = dict(jr)
    out["ref"], out["start"], out["end"] = jr["ref"] - front, jr["start"] - p.D, jr["end"] - p.D
    out["ref_off"] = jr["ref_off"][front:]
    return out


def cumulative(cols):
    """g of every read: (ref_unit0 << 16) + pos, in int64"""
    u0 = unit0(cols["ref_len"])[:-1]
    rid = np.repeat(np.arange(len(cols["ref_len"])), np.diff(cols["ref_off"]))
    return (u0[rid] << UNIT_SHIFT) + np.asarray(cols["pos"], np.int64)


def aliased_reference(cols, g):
    """the reference that holds cumulative coordinate g (-1: none): where a read would be looked for had bit 32 been lost"""
    u0 = unit0(cols["ref_len"])
    r = np.searchsorted(u0, np.asarray(g, np.int64) >> UNIT_SHIFT, side="right") - 1
    return np.where(r < len(cols["ref_len"]), r, -1)


# ---------------------------------------------------------------------------------------------------------------
# the spliced, junction and gene-count decks, near and placed (shared by tests/test_far_deck_cpu.py and
# tests/test_far_genome_gpu.py): computed once per (deck, placement), shared and never written to
# ---------------------------------------------------------------------------------------------------------------
SPLICED_DECKS = ("hand", "random", "junction")          # coverage on the first two, junctions on all three
GENE_DECKS = {"genes_hand": "hand", "junction": "junction_stretched", "genes_random": "random"}    # set -> genecounts_expected deck
TILE = 5_000


def _tiles(cols):
    """the 5-kb tiling of the deck's references, - * + cycling (tests/test_junctions_gpu.py: tiling)"""
    from bamsignals_amd.synth import tile_ranges
    rg = tile_ranges(cols["ref_len"], TILE)
    rg["strand"] = (np.arange(len(rg["rid"])) % 3 - 1).astype(np.int32)
    return rg


def _whole(cols):
    n = len(cols["ref_len"])
    return dict(rid=np.arange(n, dtype=np.int32), loc=np.zeros(n, np.int32), len=np.asarray(cols["ref_len"], np.int32),
                strand=np.zeros(n, np.int32))


Near = collections.namedtuple("Near", "cols tables ann")
Far = collections.namedtuple("Far", "placement cols tables features")


@functools.lru_cache(maxsize=None)
def near(deck):
    """(CIGAR columns, {name: range table}, annotation or None) of a deck where the suite has it.  The tables: `tiles`,
    `whole` (every reference whole) and `genes` (the junction deck's genes; elsewhere every 40th junction with 5 bases on
    either side) for the three spliced decks; the gene-count decks have their annotation alone."""
    import genecounts_expected as gx
    import junctions_expected as jx
    import spliced_expected as sx
    if deck in ("genes_hand", "genes_random"):
        cols, ann = gx.deck(GENE_DECKS[deck])
        return Near(cols, {}, ann)
    cols = {"hand": sx.hand_deck, "random": sx.random_deck, "junction": jx.junction_deck}[deck]()
    if deck == "junction":
        genes, ann = jx.junction_genes(), gx.deck("junction_stretched")[1]
        assert gx.deck("junction_stretched")[0] is cols
    else:
        jr = jx.rows(cols)
        k = np.arange(0, len(jr["start"]), 40)
        genes = dict(rid=jr["ref"][k].astype(np.int32), loc=(jr["start"][k] - 5).astype(np.int32),
                     len=(jr["end"][k] - jr["start"][k] + 11).astype(np.int32), strand=(np.arange(len(k)) % 3 - 1).astype(np.int32))
        ann = None
    return Near(cols, dict(tiles=_tiles(cols), whole=_whole(cols), genes=genes), ann)


@functools.lru_cache(maxsize=None)
def far(deck, name):
    """(placement, placed columns, placed tables, placed features or None) of a deck at the named placement; `top` is
    computed from the deck's columns, every table and the features"""
    n = near(deck)
    ranged = list(n.tables.values()) + ([n.ann.features] if n.ann is not None else [])
    p = placement(name, n.cols, *ranged)
    return Far(p, place_columns(n.cols, p), {k: place_ranges(v, p) for k, v in n.tables.items()},
               place_features(n.ann.features, p) if n.ann is not None else None)


@functools.lru_cache(maxsize=None)
def blocks(deck, name=None):
    """spliced_expected.blocks of the deck's columns, near (name None) or placed: the restatement run on those columns"""
    import spliced_expected as sx
    return sx.blocks(near(deck).cols if name is None else far(deck, name).cols)


@functools.lru_cache(maxsize=None)
def junction_rows(deck, name=None):
    import junctions_expected as jx
    return jx.rows(near(deck).cols if name is None else far(deck, name).cols)
