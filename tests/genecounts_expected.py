"""What bamGeneCounts must give, restated in numpy straight from the rule, and the decks both gene-count suites use.

The rule.  A read's BLOCKS are what ``bamCoverage(splice=True)`` covers (``spliced_expected._intervals``: the covered pieces of
its span).  Its strand ``s`` is -1 with ``flag & 0x10`` else +1, flipped when ``(flag & 0x81) == 0x81`` (a second mate).  A
feature of strand ``f`` MATCHES always (``"unstranded"``), iff ``f == 0 or f == s`` (``"forward"``), iff ``f == 0 or f == -s``
(``"reverse"``).  In this order: ``flag & 0x4`` -> unmapped; failing the library's read filter (``mapq >= mapqual``, every
``requiredF`` bit set, not every ``filteredF`` bit set; -1 filters nothing: ``junctions_expected.passes``) -> filtered; else with
H = the genes that have a matching feature of width > 0 on the read's reference sharing a base with a block: no_feature
(H empty), assigned to H's one gene, or ambiguous.  ``counts``: int64 per gene; ``summary``: assigned, ambiguous, no_feature,
filtered, unmapped.

Nothing here flattens the features: ``expected`` broadcasts every block against every feature of its reference, ``brute``
does the same with Python sets.  ``flatten_brute`` restates the library's segment tables per base, and ``decide_from_segments``
decides every read from such tables -- the trick the kernel relies on, provable on the CPU.
"""
from __future__ import annotations

import functools

import numpy as np

import junctions_expected as jx
import spliced_expected as sx

MODES = ("unstranded", "forward", "reverse")
AMBIGUOUS, NO_FEATURE, FILTERED, UNMAPPED = -1, -2, -3, -4      # a read's outcome where it is not a gene
I32 = np.int32


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def read_strand(flag):
    flag = np.asarray(flag, dtype=np.int64)
    s = np.where(flag & 0x10, -1, 1)
    return np.where((flag & 0x81) == 0x81, -s, s)


def read_blocks(cols):
    """(read, first base, last base) of every block of every read, in read order"""
    coff, cig = cols["cigar_off"], cols["cigar"]
    r, s, e = [], [], []
    for i in range(len(cols["pos"])):
        for a, b in sx._intervals(int(cols["pos"][i]), int(cols["flag"][i]), cig[coff[i]:coff[i + 1]])[0]:
            r.append(i); s.append(a); e.append(b)
    return np.asarray(r, dtype=np.int64), np.asarray(s, dtype=np.int64), np.asarray(e, dtype=np.int64)


def _blocks_cached(cols):
    key = id(cols["cigar"])
    hit = _blocks_cached.memo.get(key)
    if hit is None or hit[0] is not cols["cigar"]:
        hit = (cols["cigar"], read_blocks(cols))
        _blocks_cached.memo[key] = hit
    return hit[1]


_blocks_cached.memo = {}


def _feature_arrays(features):
    return tuple(np.asarray(features[k], dtype=np.int64) for k in ("rid", "loc", "len", "strand"))


def _matches(mode, f_strand, s):
    """features x reads?  no: elementwise over broadcast shapes"""
    if mode == "unstranded":
        return np.ones(np.broadcast(f_strand, s).shape, dtype=bool)
    want = s if mode == "forward" else -s
    return (f_strand == 0) | (f_strand == want)


def pre_outcome(cols, mapqual=0, requiredF=0, filteredF=-1):
    """UNMAPPED / FILTERED where the first two steps decide, else 0"""
    flag = cols["flag"].astype(np.int64)
    ok = jx.passes(flag, cols["mapq"].astype(np.int64), np.zeros(len(flag), np.int64), mapqual=mapqual, requiredF=requiredF,
                   filteredF=filteredF)
    return np.where(flag & 0x4, UNMAPPED, np.where(ok, 0, FILTERED))


def outcomes(cols, features, gene, n_genes, strand="unstranded", **flt):
    """Per read: its gene, or AMBIGUOUS / NO_FEATURE / FILTERED / UNMAPPED.  Every block against every feature of its
    reference by broadcasting (in slabs of blocks), then the distinct genes per read."""
    assert strand in MODES
    n = len(cols["pos"])
    gene = np.asarray(gene, dtype=np.int64)
    f_rid, f_loc, f_len, f_strand = _feature_arrays(features)
    b_read, b_start, b_end = _blocks_cached(cols)
    rid = sx._rid(cols).astype(np.int64)
    s = read_strand(cols["flag"])
    pairs = []                                                      # read * n_genes + gene of every (block, feature) hit
    for r in np.unique(rid):
        fk = np.flatnonzero((f_rid == r) & (f_len > 0))
        bk = np.flatnonzero(rid[b_read] == r)
        if not len(fk) or not len(bk):
            continue
        lo, hi = f_loc[fk][None, :], (f_loc[fk] + f_len[fk] - 1)[None, :]
        for a in range(0, len(bk), 4096):
            k = bk[a:a + 4096]
            hit = (b_start[k][:, None] <= hi) & (b_end[k][:, None] >= lo) & _matches(strand, f_strand[fk][None, :], s[b_read[k]][:, None])
            bi, fi = np.nonzero(hit)
            pairs.append(np.unique(b_read[k][bi] * n_genes + gene[fk][fi]))
    pairs = np.unique(np.concatenate(pairs)) if pairs else np.zeros(0, dtype=np.int64)
    per_read = np.bincount(pairs // max(n_genes, 1), minlength=n)
    one = np.full(n, NO_FEATURE, dtype=np.int64)
    one[pairs // max(n_genes, 1)] = pairs % max(n_genes, 1)         # (the read's gene where it has exactly one)
    out = np.where(per_read == 0, NO_FEATURE, np.where(per_read == 1, one, AMBIGUOUS))
    pre = pre_outcome(cols, **flt)
    return np.where(pre != 0, pre, out)


def tally(out, n_genes):
    """(counts, summary) of per-read outcomes"""
    out = np.asarray(out, dtype=np.int64)
    counts = np.bincount(out[out >= 0], minlength=n_genes).astype(np.int64)
    summary = np.asarray([np.count_nonzero(out >= 0)] + [np.count_nonzero(out == c) for c in (AMBIGUOUS, NO_FEATURE, FILTERED, UNMAPPED)],
                         dtype=np.int64)
    return counts, summary


def expected(cols, features, gene, n_genes, strand="unstranded", **flt):
    return tally(outcomes(cols, features, gene, n_genes, strand=strand, **flt), n_genes)


def brute_outcomes(cols, features, gene, n_genes, strand="unstranded", mapqual=0, requiredF=0, filteredF=-1):
    """The same with Python sets, one read, one block and one feature at a time (small decks)."""
    f_rid, f_loc, f_len, f_strand = (a.tolist() for a in _feature_arrays(features))
    gene = np.asarray(gene).tolist()
    by_ref = {}
    for k in range(len(f_rid)):
        by_ref.setdefault(f_rid[k], []).append(k)
    b_read, b_start, b_end = (a.tolist() for a in _blocks_cached(cols))
    blocks_of = {}
    for r, a, b in zip(b_read, b_start, b_end):
        blocks_of.setdefault(r, []).append((a, b))
    rid = sx._rid(cols).tolist()
    out = []
    for i in range(len(cols["pos"])):
        flag, mapq = int(cols["flag"][i]), int(cols["mapq"][i])
        if flag & 0x4:
            out.append(UNMAPPED)
            continue
        if mapq < mapqual or (requiredF & ~flag) != 0 or (filteredF & ~flag & 0xFFFFFFFF) == 0:
            out.append(FILTERED)
            continue
        s = -1 if flag & 0x10 else 1
        if flag & 0x81 == 0x81:
            s = -s
        found = set()
        for k in by_ref.get(rid[i], ()):
            f = f_strand[k]
            if f_len[k] <= 0 or not (strand == "unstranded" or f == 0 or f == (s if strand == "forward" else -s)):
                continue
            if gene[k] in found:
                continue
            lo, hi = f_loc[k], f_loc[k] + f_len[k] - 1
            if any(a <= hi and b >= lo for a, b in blocks_of.get(i, ())):
                found.add(gene[k])
        out.append(NO_FEATURE if not found else AMBIGUOUS if len(found) > 1 else next(iter(found)))
    return np.asarray(out, dtype=np.int64)


def brute(cols, features, gene, n_genes, strand="unstranded", **flt):
    return tally(brute_outcomes(cols, features, gene, n_genes, strand=strand, **flt), n_genes)


# ---- the segment tables, restated per base ------------------------------------------------------------------------------------
TABLES = ("unstranded", "plus", "minus")


def flatten_brute(features, gene, table, ref_len):
    """The library's segment table (``GeneModel.segments``) of references of a few thousand bases, one base at a time:
    dict(ref_off, start, end, value); every feature must lie inside its reference."""
    f_rid, f_loc, f_len, f_strand = _feature_arrays(features)
    gene = np.asarray(gene, dtype=np.int64)
    takes = {"unstranded": np.ones(len(f_rid), bool), "plus": f_strand >= 0, "minus": f_strand <= 0}[table]
    ref_off, start, end, value = [0], [], [], []
    for r, n_base in enumerate(np.asarray(ref_len).tolist()):
        at = [set() for _ in range(n_base)]
        for k in np.flatnonzero((f_rid == r) & takes & (f_len > 0)):
            for x in range(int(f_loc[k]), int(f_loc[k] + f_len[k])):
                at[x].add(int(gene[k]))
        val = [None if not g else next(iter(g)) if len(g) == 1 else -1 for g in at]
        x = 0
        while x < n_base:
            if val[x] is None:
                x += 1
                continue
            y = x
            while y + 1 < n_base and val[y + 1] == val[x]:
                y += 1
            start.append(x); end.append(y); value.append(val[x])
            x = y + 1
        ref_off.append(len(start))
    return dict(ref_off=np.asarray(ref_off, np.int64), start=np.asarray(start, I32), end=np.asarray(end, I32), value=np.asarray(value, I32))


def decide_from_segments(cols, tables, strand="unstranded", **flt):
    """Per-read outcomes from the three segment tables (name -> dict as GeneModel.segments gives it), in numpy: every block
    finds the segments it touches in its read's table by two binary searches; the read is ambiguous if one of them is -1 or
    two differ, has no feature if there is none, else belongs to the one value."""
    n = len(cols["pos"])
    b_read, b_start, b_end = _blocks_cached(cols)
    rid = sx._rid(cols).astype(np.int64)
    s = read_strand(cols["flag"])
    which = np.zeros(n, dtype=np.int64) if strand == "unstranded" else np.where((s > 0) == (strand == "forward"), 1, 2)
    big = np.iinfo(np.int64).max
    lo_read, hi_read = np.full(n, big), np.full(n, -big)
    for t, name in enumerate(TABLES):
        seg = tables[name]
        val = np.concatenate([seg["value"].astype(np.int64), [0]])          # (reduceat wants its indices inside)
        for r in range(len(seg["ref_off"]) - 1):
            s0, s1 = int(seg["ref_off"][r]), int(seg["ref_off"][r + 1])
            bk = np.flatnonzero((rid[b_read] == r) & (which[b_read] == t))
            if s0 == s1 or not len(bk):
                continue
            k0 = s0 + np.searchsorted(seg["end"][s0:s1], b_start[bk], "left")
            k1 = s0 + np.searchsorted(seg["start"][s0:s1], b_end[bk], "right")
            some = k1 > k0
            bk, k0, k1 = bk[some], k0[some], k1[some]
            if not len(bk):
                continue
            idx = np.stack([k0, k1], axis=1).reshape(-1)
            np.minimum.at(lo_read, b_read[bk], np.minimum.reduceat(val, idx)[::2])
            np.maximum.at(hi_read, b_read[bk], np.maximum.reduceat(val, idx)[::2])
    out = np.where(hi_read == -big, NO_FEATURE, np.where((lo_read < 0) | (lo_read != hi_read), AMBIGUOUS, lo_read))
    pre = pre_outcome(cols, **flt)
    return np.where(pre != 0, pre, out)


# ---- decks ------------------------------------------------------------------------------------------------------------------
def _rows_of(cols):
    rid = sx._rid(cols)
    coff, cig = cols["cigar_off"], cols["cigar"]
    return [(int(rid[i]), int(cols["pos"][i]), int(cols["flag"][i]), int(cols["mapq"][i]), int(cols["tlen"][i]),
             np.asarray(cig[coff[i]:coff[i + 1]], dtype=np.uint32)) for i in range(len(cols["pos"]))]


def _columns_of(ref_len, rows):
    """rows (rid, pos, flag, mapq, tlen, packed operations) -> CIGAR columns, stably sorted by (rid, pos)"""
    rows = sorted(rows, key=lambda r: (r[0], r[1]))
    rid = np.asarray([r[0] for r in rows], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum([len(r[5]) for r in rows])]).astype(np.int64)
    cols = dict(ref_len=np.asarray(ref_len, dtype=I32), ref_off=np.searchsorted(rid, np.arange(len(ref_len) + 1)).astype(np.int64),
                pos=np.asarray([r[1] for r in rows], dtype=I32), flag=np.asarray([r[2] for r in rows], dtype=np.uint16),
                mapq=np.asarray([r[3] for r in rows], dtype=np.uint8), tlen=np.asarray([r[4] for r in rows], dtype=I32),
                cigar_off=coff, cigar=np.concatenate([r[5] for r in rows]).astype(np.uint32) if rows else np.zeros(0, np.uint32))
    cols["end"] = sx.ends(cols)
    for a in cols.values():
        a.setflags(write=False)
    return cols


class Annotation:
    """features (rid, loc, len, strand as int32 arrays), gene (index per feature), labels (one per gene)"""

    def __init__(self, feats, labels=None):
        # feats: (label, rid, first base, last base, strand); extra labels: genes without a feature
        self.labels = list(dict.fromkeys([f[0] for f in feats] + list(labels or [])))
        lut = {g: k for k, g in enumerate(self.labels)}
        self.gene = np.asarray([lut[f[0]] for f in feats], dtype=I32)
        self.features = dict(rid=np.asarray([f[1] for f in feats], I32), loc=np.asarray([f[2] for f in feats], I32),
                             len=np.asarray([f[3] - f[2] + 1 for f in feats], I32), strand=np.asarray([f[4] for f in feats], I32))
        self.n_genes = len(self.labels)
        for a in (self.gene, *self.features.values()):
            a.setflags(write=False)

    def index(self, label):
        return self.labels.index(label)

    def twice_and_reversed(self):
        """the features given twice and reversed, with the same genes: nothing may change"""
        other = Annotation.__new__(Annotation)
        other.labels, other.n_genes = self.labels, self.n_genes
        other.gene = np.concatenate([self.gene, self.gene, self.gene[::-1]])
        other.features = {k: np.concatenate([v, v, v[::-1]]) for k, v in self.features.items()}
        return other


HAND_REF_LEN = sx.HAND_REF_LEN + [50_000, 50_000]       # 3: features and no reads; 4: reads and no features; 1: neither
N_STEPPING = 1_100                                      # single-exon genes inside one read's intron
LONG_LAST = 100_000 + sx.LONG_OPS - 2                   # the first base of the long read's last block


@functools.lru_cache(maxsize=1)
def hand():
    """(columns, Annotation, {name: read index}): spliced_expected.hand_deck() with the reads the gene-count cases need added
    on reference 0 from base 10,000 on (nothing of the hand deck lies there) and on reference 4."""
    extra = [                                            # name, (rid, pos, flag, mapq, tlen, cigar)
        ("before_start", (0, 10_000, 0, 60, 0, "50M")), ("on_start", (0, 10_200, 0, 60, 0, "50M")),
        ("behind_end", (0, 10_400, 0, 60, 0, "50M")), ("on_end", (0, 10_600, 0, 60, 0, "50M")),
        ("two_exons", (0, 11_000, 16, 60, 0, "30M100N30M")), ("two_genes", (0, 12_000, 0, 60, 0, "30M100N30M")),
        ("inside_ambig", (0, 13_100, 0, 60, 0, "50M")),
        ("over_nested", (0, 14_050, 0, 60, 0, "51M899N50M")), ("in_nested", (0, 14_450, 0, 60, 0, "50M")),
        ("touch_left", (0, 16_050, 0, 60, 0, "50M")), ("touch_both", (0, 16_080, 0, 60, 0, "40M")), ("touch_right", (0, 16_100, 16, 60, 0, "50M")),
        ("transcripts", (0, 17_060, 0, 60, 0, "50M")),
        ("anti_fwd", (0, 18_150, 0, 60, 0, "50M")), ("anti_rev", (0, 18_150, 16, 60, 0, "50M")),
        ("star_fwd", (0, 19_010, 0, 60, 0, "50M")), ("star_rev", (0, 19_010, 16, 60, 0, "50M")),
        ("mate2_rev", (0, 20_010, 0x81 | 0x10, 60, 0, "50M")), ("mate2_fwd", (0, 20_020, 0x81, 60, 0, "50M")),
        ("mate1_rev", (0, 20_030, 0x41 | 0x10, 60, 0, "50M")),
        ("long_intron", (0, 30_000, 0, 60, 0, "50M60000N50M")), ("stepping_398", (0, 50_005, 0, 60, 0, "10M")),
        ("no_features_here", (4, 100, 0, 60, 0, "50M")),
    ]
    base = sx.hand_deck()
    rows = _rows_of(base) + [(r[0], r[1], r[2], r[3], r[4], np.asarray(sx.cigar(r[5]), dtype=np.uint32)) for _, r in extra]
    cols = _columns_of(HAND_REF_LEN, rows)
    rid = sx._rid(cols)
    where = {}
    for name, r in extra:
        k = np.flatnonzero((rid == r[0]) & (cols["pos"] == r[1]) & (cols["flag"] == r[2]))
        assert len(k) == 1, name
        where[name] = int(k[0])
    k = np.flatnonzero((rid == 2) & (cols["pos"] == 100_000))
    assert len(k) == 1
    where["long_read"] = int(k[0])
    feats = [                                            # label, rid, first base, last base, strand
        ("E0", 0, 9_980, 9_999, 1), ("E1", 0, 10_180, 10_200, 1), ("E2", 0, 10_450, 10_470, 1), ("E3", 0, 10_649, 10_670, 1),
        ("Z", 0, 10_010, 10_009, 1),                     # width 0, inside before_start's block
        ("X2", 0, 10_990, 11_029, -1), ("X2", 0, 11_130, 11_200, -1),
        ("C1", 0, 11_990, 12_010, 1), ("C2", 0, 12_140, 12_170, 1),
        ("D1", 0, 13_000, 13_200, 1), ("D2", 0, 13_050, 13_300, 1),
        ("OUTER", 0, 14_000, 14_100, 1), ("OUTER", 0, 15_000, 15_100, 1), ("INNER", 0, 14_400, 14_600, 1),
        ("F1", 0, 16_000, 16_099, 1), ("F2", 0, 16_100, 16_199, -1),
        ("T", 0, 17_000, 17_100, 1), ("T", 0, 17_050, 17_200, 1),
        ("P", 0, 18_000, 18_300, 1), ("M", 0, 18_100, 18_400, -1),
        ("S", 0, 19_000, 19_100, 0),
        ("J", 0, 20_000, 20_200, 1),
        ("KA", 0, 29_990, 30_010, 1), ("KA", 0, 90_060, 90_080, 1),
        ("W1", 0, 90, 460, 1), ("W2", 0, 2_150, 2_260, -1), ("W3", 2, 0, 150, 0), ("W4", 2, 1_030, 1_060, 1),
        ("L", 2, LONG_LAST, LONG_LAST + 12, 1), ("L_GAP", 2, LONG_LAST - 1, LONG_LAST - 1, 1),
        ("N1", 3, 100, 500, 1),
    ]
    feats += [(f"K{j}", 0, 30_100 + 50 * j, 30_119 + 50 * j, 1 if j % 2 else -1) for j in range(N_STEPPING)]
    return cols, Annotation(feats, labels=["NO_FEATURE_GENE"]), where


def _replay_exons(seed):
    """The exons of junctions_expected._deck(seed): its generator replayed draw for draw (the reads' draws are made and
    thrown away).  test_genecounts_cpu checks the replay against junction_genes()."""
    rng = np.random.default_rng(seed)
    genes = []
    for rid in (0, 2):
        for g, n_reads in enumerate(jx.READS_PER_GENE):
            while True:
                n_exon = int(rng.integers(3, 9))
                exons = rng.integers(30, 201, n_exon)
                introns = np.exp(rng.uniform(np.log(80), np.log(20_000), n_exon - 1)).astype(np.int64).clip(80, 20_000)
                if exons.sum() + introns.sum() <= jx.GENE_SLOT - 2_000:
                    break
            first = g * jx.GENE_SLOT + 1_000 + int(rng.integers(0, 500))
            ex_start = first + np.concatenate([[0], np.cumsum(exons[:-1] + introns)])
            ex_end = ex_start + exons - 1
            minus = bool(rng.integers(0, 2))
            genes.append((rid, [int(x) for x in ex_start], [int(x) for x in ex_end], -1 if minus else 1))
            for _ in range(n_reads):
                kept = [0] + [k for k in range(1, n_exon - 1) if rng.random() >= 0.15] + [n_exon - 1]
                t_len = int(exons[kept].sum())
                rng.integers(0, t_len - min(jx.READ_BASES, t_len) + 1)
                rng.random(); rng.random(); rng.choice([0, 3, 30, 60])
    return genes


@functools.lru_cache(maxsize=2)
def junction(stretched=False):
    """(columns, Annotation) of junctions_expected.junction_deck(): its twenty genes' exons, on the gene's strand (10 % of the
    reads lie on the other one).  ``stretched``: every gene's last exon reaches 10 bases into the first exon of the next gene
    on its reference, so the reads of that exon are ambiguous and break the runs of equal outcomes."""
    genes = _replay_exons(jx.DECK_SEED)
    feats = []
    for k, (rid, starts, ends, strand) in enumerate(genes):
        ends = list(ends)
        if stretched and k + 1 < len(genes) and genes[k + 1][0] == rid:
            ends[-1] = genes[k + 1][1][0] + 9
        feats += [(f"g{rid}_{k % len(jx.READS_PER_GENE)}", rid, a, b, strand) for a, b in zip(starts, ends)]
    return jx.junction_deck(), Annotation(feats)


RANDOM_GENES = 300


@functools.lru_cache(maxsize=1)
def random():
    """(columns, Annotation): spliced_expected.random_deck()'s 5,000 reads -- its flags carry only 0x10 and 0x400, so a seeded
    2 % are made unmapped (0x4) and 30 % mates of a pair (0x1, 0x40 or 0x80, nine in ten proper: 0x2) in a copy -- against
    300 seeded genes of 1-8 exons of 50-400 bases on any strand, overlapping freely."""
    base = sx.random_deck()
    rng = np.random.default_rng(20261021)
    n = len(base["pos"])
    flag = base["flag"].astype(np.uint16).copy()
    flag[rng.random(n) < 0.02] |= 0x4
    paired = rng.random(n) < 0.30
    flag[paired] |= np.where(rng.random(n) < 0.5, 0x41, 0x81).astype(np.uint16)[paired]
    flag[paired & (rng.random(n) < 0.9)] |= 0x2
    cols = dict(base)
    cols["flag"] = flag
    for a in cols.values():
        a.setflags(write=False)
    feats = []
    for g in range(RANDOM_GENES):
        rid, strand = int(rng.integers(0, 3)), int(rng.choice([-1, 0, 1], p=[0.45, 0.1, 0.45]))
        at = int(rng.integers(0, 190_000))
        for _ in range(int(rng.integers(1, 9))):
            w = int(rng.integers(50, 401))
            if at + w > 200_000:
                break
            feats.append((f"r{g}", rid, at, at + w - 1, strand))
            at += w + int(rng.integers(-30, 3_000))         # (now and then an exon overlaps the one before)
    return cols, Annotation(feats, labels=[f"r{g}" for g in range(RANDOM_GENES)])


def deck(name):
    """name -> (columns, Annotation)"""
    if name == "hand":
        return hand()[:2]
    return {"junction": junction, "junction_stretched": lambda: junction(True), "random": random}[name]()


DECKS = ("hand", "junction", "junction_stretched", "random")
