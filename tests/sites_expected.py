"""What bamSites must give, restated in numpy and once more one cell at a time, and the sites deck both site suites use.

Semantics (include/bamsignals_abi.h, restated).  A site is decided from the cells of a range exactly as the nucleotide counts
define them (tests/nucleotides_expected.py: after a ``-`` range's reversal and complement, with the same filters).  For a cell
let ``c[0..5]`` be the channels ``A C G T N -``, the two planes summed with ss, and ``D`` their sum.  The BASE channel ``b`` is
``ref[cell]`` -- a code 0 .. 4 per cell, range after range as the range reads; a cell whose ref is 4 is never a site -- or,
without ref, the first channel of all six with the largest count.  The ALT channel ``a`` is the first channel with the largest
count among those in ``alt_mask``, ``b`` excluded (no such channel: no site).  The cell is a site iff ``D >= min_depth``,
``c[a] >= min_alt`` and ``c[a] * den >= num * D``.  The result: ``seg_off`` (n + 1), ``pos`` (the cell's index in its range,
ascending), ``alleles`` (``b | a << 8``), ``counts`` (the cell's counts as the nucleotide call reports them: ``(6,)`` a site,
``(2, 6)`` with ss).

PARAMETERS are a dict: min_depth, min_alt, num, den, alt_mask.
"""
from __future__ import annotations

import functools

import numpy as np

import nucleotides_expected as nx

MASK_WITH_DELETIONS, MASK_BASES = 0x2F, 0x0F


def prm(min_depth, min_alt, num, den, alt_mask=MASK_WITH_DELETIONS):
    return dict(min_depth=min_depth, min_alt=min_alt, num=num, den=den, alt_mask=alt_mask)


def _empty(n, ss):
    return dict(seg_off=np.zeros(n + 1, dtype=np.int64), pos=np.zeros(0, dtype=np.int32), alleles=np.zeros(0, dtype=np.int32),
                counts=np.zeros((0, 2, 6) if ss else (0, 6), dtype=np.int32))


# ---- the restatement: numpy over the dense cells -------------------------------------------------------------------------------
def expected_sites(dense, ref, p):
    """dense: one (6, w) or (2, 6, w) int32 array per range (nucleotides_expected.expected); ref: None, or one uint8 array of w
    codes per range; p: the parameters.  -> dict(seg_off, pos, alleles, counts)"""
    n = len(dense)
    ss = n > 0 and dense[0].ndim == 3
    seg, pos, alleles, counts = [0], [], [], []
    for i, cells in enumerate(dense):
        cells = np.asarray(cells)
        c = cells.astype(np.int64).sum(axis=0) if ss else cells.astype(np.int64)         # (6, w)
        w = c.shape[1]
        depth = c.sum(axis=0)
        if ref is None:
            b = np.argmax(c, axis=0)                            # (the first of the largest)
            known = np.ones(w, dtype=bool)
        else:
            b = np.asarray(ref[i], dtype=np.int64)
            assert b.shape == (w,) and (w == 0 or b.max() <= 4)
            known = b != 4
        allowed = ((p["alt_mask"] >> np.arange(6)) & 1).astype(bool)[:, None] & (np.arange(6)[:, None] != b[None, :])
        masked = np.where(allowed, c, -1)
        a = np.argmax(masked, axis=0)
        ca = masked[a, np.arange(w)] if w else np.zeros(0, dtype=np.int64)
        site = known & (depth >= p["min_depth"]) & (ca >= p["min_alt"]) & (ca * p["den"] >= p["num"] * depth) & allowed.any(axis=0)
        at = np.flatnonzero(site)
        pos.append(at.astype(np.int32))
        alleles.append((b[at] | a[at] << 8).astype(np.int32))
        counts.append(np.moveaxis(cells[..., at], -1, 0).astype(np.int32))
        seg.append(seg[-1] + len(at))
    if not n:
        return _empty(0, False)
    return dict(seg_off=np.asarray(seg, dtype=np.int64), pos=np.concatenate(pos), alleles=np.concatenate(alleles),
                counts=np.concatenate(counts, axis=0))


# ---- the same, one cell at a time in plain Python (shares no code with the above) ---------------------------------------------------
def brute_sites(dense, ref, p):
    seg, pos, alleles, counts = [0], [], [], []
    ss = len(dense) > 0 and np.asarray(dense[0]).ndim == 3
    for i, cells in enumerate(dense):
        lst = np.asarray(cells).tolist()
        w = np.asarray(cells).shape[-1]
        for j in range(w):
            c = [lst[0][k][j] + lst[1][k][j] for k in range(6)] if ss else [lst[k][j] for k in range(6)]
            d = sum(c)
            if ref is None:
                b = 0
                for k in range(1, 6):
                    if c[k] > c[b]:
                        b = k
            else:
                b = int(ref[i][j])
                if b == 4:
                    continue
            a = None
            for k in range(6):
                if k != b and p["alt_mask"] & (1 << k) and (a is None or c[k] > c[a]):
                    a = k
            if a is None or d < p["min_depth"] or c[a] < p["min_alt"] or c[a] * p["den"] < p["num"] * d:
                continue
            pos.append(j)
            alleles.append(b | a << 8)
            counts.append([[lst[pl][k][j] for k in range(6)] for pl in range(2)] if ss else [lst[k][j] for k in range(6)])
        seg.append(len(pos))
    if not pos:
        return _empty(len(dense), ss)
    return dict(seg_off=np.asarray(seg, dtype=np.int64), pos=np.asarray(pos, dtype=np.int32), alleles=np.asarray(alleles, dtype=np.int32),
                counts=np.asarray(counts, dtype=np.int32))


def same_sites(got, want):
    """got: (seg_off, pos, alleles, counts) or a dict of them"""
    if not isinstance(got, dict):
        got = dict(zip(("seg_off", "pos", "alleles", "counts"), got))
    return all(np.asarray(got[k]).shape == np.asarray(want[k]).shape and np.array_equal(got[k], want[k])
               for k in ("seg_off", "pos", "alleles", "counts"))


def flat_ref(ref):
    """the per-range codes as the library takes them: one uint8 array, range after range"""
    return np.concatenate([np.asarray(r, dtype=np.uint8) for r in ref]) if len(ref) else np.zeros(0, dtype=np.uint8)


def random_ref(rg, seed=3):
    """a reference for any deck: seeded codes 0 .. 4 per cell (N one time in ten), one array per range"""
    rng = np.random.default_rng(seed)
    return [rng.choice(5, int(w), p=[.225, .225, .225, .225, .1]).astype(np.uint8) for w in rg["len"]]


# ---- the sites deck ------------------------------------------------------------------------------------------------------------
SITES_NAMES = ["chrS", "chrNone"]
SITES_REF_LEN = [8_192, 5_000]
READ_LEN, STEP, PER_START = 50, 5, 3            # reads of 50 bases, three at every fifth base: depth 30 inside, 3 more every 5 bases at the start
DEPTH = READ_LEN // STEP * PER_START
NAMED = prm(9, 2, 1, 5)                         # the parameters the planted cells are named for
_COMP = np.array([3, 2, 1, 0, 4, 5])
_CODE_OF_CHANNEL = [1, 2, 4, 8, 15]


@functools.lru_cache(maxsize=1)
def sites_deck():
    """(records, ranges, genome, planted): reads that copy a seeded reference of 8 kb but where a cell is planted.  genome: the
    reference's channel codes (0 .. 3) with the planted N (4) -- as a '+' range reads it.  planted: name -> dict(x = the genomic
    base, site = is it one under NAMED with the reference, and where it is: base, alt, alt_count, depth)."""
    rng = np.random.default_rng(20261022)
    L = SITES_REF_LEN[0]
    genome = rng.integers(0, 4, L).astype(np.uint8)
    starts = [s for s in range(0, L - READ_LEN + 1, STEP) for _ in range(PER_START)]
    edits = [dict() for _ in starts]            # per read: genomic base -> a channel 0 .. 4, "del" or "skip"
    planted = {}

    def covering(x):
        return [k for k, s in enumerate(starts) if s <= x < s + READ_LEN]

    def plant(name, x, shown, site=True, ref_n=False):
        """shown: [(what, number of reads)] -- the first reads that cover x take them in turn; channels are given relative to
        the reference: +k is the channel (ref + k) % 4"""
        reads = covering(x)
        at = 0
        tally = {}
        for what, k in shown:
            ch = what if isinstance(what, str) else (int(genome[x]) + what) % 4
            for r in reads[at:at + k]:
                edits[r][x] = ch
            at += k
            tally[5 if ch == "del" else ch] = k
        assert at <= len(reads)
        skipped = tally.pop("skip", 0)
        depth = len(reads) - skipped
        alt = max(tally, key=lambda ch: (tally[ch], -ch))        # the most reads, the first channel on a tie
        # (alts: every channel that shares the largest number -- a '-' range sees them complemented, and its first is another)
        planted[name] = dict(x=x, site=site, base=int(genome[x]), alt=alt, alts=[ch for ch in tally if tally[ch] == tally[alt]],
                             alt_count=tally[alt], depth=depth, ref_n=ref_n)

    plant("het", 200, [(1, 15)])
    plant("hom", 300, [(2, 30)])
    plant("deletion", 400, [("del", 12)])
    plant("alt_tie", 500, [(1, 8), (2, 8)])                      # two alts of 8 reads each: the first channel of the two wins
    plant("major_tie", 600, [(1, 15)])                           # 15 : 15 -- without a reference the first channel is the base
    plant("exact_fraction", 700, [(3, 6)])                       # 6 * 5 == 1 * 30
    plant("one_short", 800, [(3, 5)], site=False)                # 5 * 5 < 30
    plant("ref_n", 900, [(1, 10)], site=False, ref_n=True)       # a mismatch under a reference N
    plant("at_min_depth", 10, [(1, 3)])                          # depth 9 == min_depth
    plant("below_min_depth", 12, [(1, 3), ("skip", 1)], site=False)     # 8 reads: one of the nine skips the base (N)
    # the big ranges [2000, 2000 + 3 * 1024 + 1): cells 0, 1023, 1024 and the last, as a '+' and as a '-' range reads
    for name, x in (("plus_cell_0", 2000), ("plus_cell_1023", 3023), ("plus_cell_1024", 3024), ("plus_last", 5072),
                    ("minus_cell_1023", 5072 - 1023), ("minus_cell_1024", 5072 - 1024)):
        plant(name, x, [(2, 10)])
    ops, codes, quals, flags = [], [], [], []
    for k, s in enumerate(starts):
        o, c = [], []
        for x in range(s, s + READ_LEN):
            e = edits[k].get(x)
            op = 2 if e == "del" else 3 if e == "skip" else 0
            if o and (o[-1] & 0xF) == op:
                o[-1] += 1 << 4
            else:
                o.append(1 << 4 | op)
            if op == 0:
                c.append(_CODE_OF_CHANNEL[int(genome[x]) if e is None else e])
        ops.append(o); codes.append(np.asarray(c, dtype=np.uint8)); quals.append(np.full(len(c), 30, dtype=np.uint8))
        flags.append(16 if k % 2 else 0)
    n = len(starts)
    rec = nx.columns(SITES_REF_LEN, np.zeros(n), starts, flags, np.full(n, 40), np.zeros(n), ops, codes, quals)
    T = nx.TILE
    rg = [   # (rid, loc, len, strand)
        (0, 200, 1, 1), (0, 200, 1, -1), (0, 201, 1, 0),                                    # width 1: a site, and none
        (0, 0, T - 1, 1), (0, 0, T, -1), (0, 0, T + 1, 0),
        (0, 2000, 3 * T + 1, 1), (0, 2000, 3 * T + 1, -1), (0, 2000, 3 * T + 1, 1),           # every strand, a duplicate
        (0, 100, 0, 1),                                                                      # width 0
        (0, 150, 400, 1), (0, 1000, 500, 1), (0, 580, 400, -1),                              # no site between two with sites
        (1, 0, 2_000, 1), (0, 8_000, 500, 1),                                                # a reference without reads; past the end
    ]
    rg = dict(zip(("rid", "loc", "len", "strand"), (np.asarray(c, dtype=np.int32) for c in zip(*rg))))
    ref_plus = genome.copy()
    ref_plus[planted["ref_n"]["x"]] = 4
    for a in list(rec.values()) + list(rg.values()) + [ref_plus]:
        a.setflags(write=False)
    return rec, rg, ref_plus, planted


def deck_ref(rg, genome_codes, none_code=0):
    """the sites deck's reference for its ranges, one uint8 array per range as the range reads: the genome's codes, for a '-' range
    reversed and complemented, beyond the genome's end and on the reference without reads ``none_code``"""
    out = []
    for rid, loc, w, strand in zip(*(np.asarray(rg[k]).tolist() for k in ("rid", "loc", "len", "strand"))):
        r = np.full(w, none_code, dtype=np.uint8)
        if rid == 0:
            k = max(min(len(genome_codes) - loc, w), 0)
            r[:k] = genome_codes[loc:loc + k]
        out.append(_COMP[r[::-1]].astype(np.uint8) if strand < 0 else r)
    return out


def cell_of(rg, i, x):
    """the cell of genomic base x in range i, as the range reads"""
    loc, w = int(rg["loc"][i]), int(rg["len"][i])
    return loc + w - 1 - x if rg["strand"][i] < 0 else x - loc


# ---- the decks by name, their dense cells computed once ---------------------------------------------------------------------------
FILTERS = (dict(), dict(mapqual=30, filteredF=0x400))          # the two filter sets of the nucleotide suite


def deck(name):
    """(records, ranges, names)"""
    if name == "hand":
        return (*nx.hand_deck(), nx.HAND_NAMES)
    if name == "random":
        return (*nx.random_deck(), nx.RANDOM_NAMES)
    rec, rg, _, _ = sites_deck()
    return rec, rg, SITES_NAMES


def ref_of(name):
    rec, rg, _ = deck(name)
    if name == "sites":
        return deck_ref(rg, sites_deck()[2])
    return random_ref(rg)


_dense = {}


def dense(name, ss, min_base_qual=0, **flt):
    """nucleotides_expected.expected on the deck's own ranges, computed once per filter (with ss; without it the planes add up)"""
    key = (name, min_base_qual, tuple(sorted(flt.items())))
    if key not in _dense:
        rec, rg, _ = deck(name)
        _dense[key] = nx.expected(rec, rg, ss=True, min_base_qual=min_base_qual, **flt)
        for a in _dense[key]:
            a.setflags(write=False)
    return _dense[key] if ss else [a.sum(axis=0, dtype=np.int32) for a in _dense[key]]
