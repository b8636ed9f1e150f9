"""What bamJunctions must give, restated in numpy, and the deck with planted multiplicities both junction suites use.

A junction row is one gap of one read, exactly as ``spliced_expected._intervals`` cuts them: (reference, start, end, the read's
flag and mapq, anchor).  ``anchor = min(left, right)``: the length of the covered piece that ends at ``start - 1`` and of the
one that begins at ``end + 1`` (``_intervals`` merges M D = X into maximal pieces: D counts, I does not), 0 where there is no
such piece.  The rows are stably sorted by (reference, start, end).

A row belongs to a range iff it is on its reference, ``start >= loc``, ``end <= loc + len - 1``, it passes the flag / mapq
filter as a read passes it in every other call (``mapq >= mapqual``, every ``requiredF`` bit set, and NOT every ``filteredF``
bit set: the reference's ``filteredF & ~flag`` test -- for a mask of one bit that is ``flag & filteredF == 0``, and -1 filters
nothing), and ``anchor >= min_anchor``.  Per range: the distinct (start, end) ascending, the number of rows of each -- with ss
split into sense (the row's 0x10 bit agrees with the range's strand, ``*`` as ``+``) and antisense -- and the largest anchor.
"""
from __future__ import annotations

import functools

import numpy as np

import spliced_expected as sx


def rows(cols):
    """The junction rows of CIGAR columns: dict(ref_off, ref, start, end, flag, mapq, anchor), sorted by (ref, start, end)."""
    rid = sx._rid(cols)
    coff, cig = cols["cigar_off"], cols["cigar"]
    ref, start, end, flag, mapq, anchor = [], [], [], [], [], []
    for i in range(len(cols["pos"])):
        covered, gaps, _ = sx._intervals(int(cols["pos"][i]), int(cols["flag"][i]), cig[coff[i]:coff[i + 1]])
        if not gaps:
            continue
        ends_at = {b: b - a + 1 for a, b in covered}
        begins_at = {a: b - a + 1 for a, b in covered}
        for a, b in gaps:
            ref.append(int(rid[i])); start.append(a); end.append(b)
            flag.append(int(cols["flag"][i])); mapq.append(int(cols["mapq"][i]))
            anchor.append(min(ends_at.get(a - 1, 0), begins_at.get(b + 1, 0)))
    ref, start, end = (np.asarray(x, dtype=np.int64) for x in (ref, start, end))
    order = np.lexsort((end, start, ref)) if len(ref) else np.zeros(0, dtype=np.int64)          # (lexsort is stable)
    n_ref = len(cols["ref_len"])
    out = dict(ref=ref[order], start=start[order], end=end[order], flag=np.asarray(flag, dtype=np.int64)[order],
               mapq=np.asarray(mapq, dtype=np.int64)[order], anchor=np.asarray(anchor, dtype=np.int64)[order])
    out["ref_off"] = np.searchsorted(out["ref"], np.arange(n_ref + 1)).astype(np.int64)
    return out


def passes(flag, mapq, anchor, mapqual=0, requiredF=0, filteredF=-1, min_anchor=0):
    nf = ~np.asarray(flag, dtype=np.int64)
    return (mapq >= mapqual) & ((requiredF & nf) == 0) & ((filteredF & nf & 0xFFFFFFFF) != 0) & (anchor >= min_anchor)


def expected(jr, rg, ss=False, **flt):
    """(seg_off, start, end, count, max_anchor) of the ranges rg (rid, loc, len, strand; 0-based), via np.unique."""
    seg_off, S, E, C, A = [0], [], [], [], []
    for rid, loc, ln, strand in zip(*(np.asarray(rg[k], dtype=np.int64) for k in ("rid", "loc", "len", "strand"))):
        n_here = 0
        if ln > 0:
            r0, r1 = jr["ref_off"][rid], jr["ref_off"][rid + 1]
            a = r0 + np.searchsorted(jr["start"][r0:r1], loc, "left")
            b = r0 + np.searchsorted(jr["start"][r0:r1], loc + ln - 1, "right")
            sl = slice(a, b)
            keep = (jr["end"][sl] <= loc + ln - 1) & passes(jr["flag"][sl], jr["mapq"][sl], jr["anchor"][sl], **flt)
            if np.any(keep):
                s, e, f, an = jr["start"][sl][keep], jr["end"][sl][keep], jr["flag"][sl][keep], jr["anchor"][sl][keep]
                pairs, inv = np.unique(np.stack([s, e], axis=1), axis=0, return_inverse=True)
                inv = inv.reshape(-1)
                anti = ((f & 16) != 0) != (strand < 0) if ss else np.zeros(len(s), bool)
                sense_n = np.bincount(inv, weights=~anti, minlength=len(pairs)).astype(np.int64)
                anti_n = np.bincount(inv, weights=anti, minlength=len(pairs)).astype(np.int64)
                best = np.zeros(len(pairs), dtype=np.int64)
                np.maximum.at(best, inv, an)
                S.append(pairs[:, 0]); E.append(pairs[:, 1]); A.append(best)
                C.append(np.stack([sense_n, anti_n], axis=1) if ss else sense_n)
                n_here = len(pairs)
        seg_off.append(seg_off[-1] + n_here)
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, dtype=np.int64)      # noqa: E731
    return (np.asarray(seg_off, dtype=np.int64), cat(S, 0), cat(E, 0), cat(C, (0, 2) if ss else 0), cat(A, 0))


def brute(jr, rg, ss=False, mapqual=0, requiredF=0, filteredF=-1, min_anchor=0):
    """The same, one range and one row at a time with a dictionary (small inputs)."""
    seg_off, S, E, C, A = [0], [], [], [], []
    n_rows = len(jr["start"])
    for rid, loc, ln, strand in zip(*(np.asarray(rg[k]).tolist() for k in ("rid", "loc", "len", "strand"))):
        found = {}
        for k in range(n_rows):
            if jr["ref"][k] != rid or jr["start"][k] < loc or jr["end"][k] > loc + ln - 1:
                continue
            flag, mapq, anchor = int(jr["flag"][k]), int(jr["mapq"][k]), int(jr["anchor"][k])
            if mapq < mapqual or (requiredF & ~flag) != 0 or (filteredF & ~flag & 0xFFFFFFFF) == 0 or anchor < min_anchor:
                continue
            cell = found.setdefault((int(jr["start"][k]), int(jr["end"][k])), [0, 0, 0])
            cell[1 if ss and bool(flag & 16) != (strand < 0) else 0] += 1
            cell[2] = max(cell[2], anchor)
        for (s, e), cell in sorted(found.items()):
            S.append(s); E.append(e); C.append(cell[:2] if ss else cell[0]); A.append(cell[2])
        seg_off.append(len(S))
    return (np.asarray(seg_off, dtype=np.int64), np.asarray(S, dtype=np.int64), np.asarray(E, dtype=np.int64),
            np.asarray(C, dtype=np.int64).reshape((-1, 2) if ss else (-1,)), np.asarray(A, dtype=np.int64))


def same(got, want):
    """are two results (seg_off, start, end, count, max_anchor) equal, shapes and all?"""
    return len(got) == len(want) == 5 and all(np.asarray(g).shape == np.asarray(w).shape and np.array_equal(g, w)
                                              for g, w in zip(got, want))


# ---- the deck with planted multiplicities --------------------------------------------------------------------------------
DECK_REF_LEN = [500_000, 5_000, 500_000]        # the middle reference stays empty
READS_PER_GENE = (1, 3, 63, 64, 65, 255, 256, 257, 1_100, 4_000)
GENE_SLOT = 48_000                              # every gene lies in a slot of its own
READ_BASES = 100
DECK_SEED = 1


@functools.lru_cache(maxsize=4)
def _deck(seed):
    rng = np.random.default_rng(seed)
    reads, genes = [], []
    for rid in (0, 2):
        for g, n_reads in enumerate(READS_PER_GENE):
            while True:         # 3-8 exons of 30-200 bases, introns of 80-20,000 (log-uniform), redrawn until the slot holds them
                n_exon = int(rng.integers(3, 9))
                exons = rng.integers(30, 201, n_exon)
                introns = np.exp(rng.uniform(np.log(80), np.log(20_000), n_exon - 1)).astype(np.int64).clip(80, 20_000)
                if exons.sum() + introns.sum() <= GENE_SLOT - 2_000:
                    break
            first = g * GENE_SLOT + 1_000 + int(rng.integers(0, 500))
            ex_start = first + np.concatenate([[0], np.cumsum(exons[:-1] + introns)])
            ex_end = ex_start + exons - 1
            minus = bool(rng.integers(0, 2))
            genes.append((rid, int(ex_start[0]), int(ex_end[-1]), -1 if minus else 1))
            for _ in range(n_reads):
                kept = [0] + [k for k in range(1, n_exon - 1) if rng.random() >= 0.15] + [n_exon - 1]
                t_len = int(exons[kept].sum())
                ln = min(READ_BASES, t_len)
                at = int(rng.integers(0, t_len - ln + 1))
                pos, text, left, last_end = None, "", ln, None
                for k in kept:
                    if at >= exons[k]:
                        at -= int(exons[k])
                        continue
                    take = min(int(exons[k]) - at, left)
                    if pos is None:
                        pos = int(ex_start[k]) + at
                    else:
                        text += f"{int(ex_start[k]) - last_end - 1}N"
                    text += f"{take}M"
                    last_end = int(ex_start[k]) + at + take - 1
                    left -= take
                    at = 0
                    if left == 0:
                        break
                rev = minus != (rng.random() < 0.10)
                flag = (16 if rev else 0) | (0x400 if rng.random() < 0.03 else 0)
                reads.append((rid, pos, flag, int(rng.choice([0, 3, 30, 60])), 0, text))
    reads.sort(key=lambda r: (r[0], r[1]))      # (stable: ties keep the order they were drawn in)
    cols = sx.columns(DECK_REF_LEN, reads)
    for a in cols.values():
        a.setflags(write=False)
    return cols, tuple(genes)


def junction_deck(seed=DECK_SEED):
    """CIGAR columns: ten genes on each of references 0 and 2 with 1 .. 4,000 reads of 100 transcript bases each; every inner
    exon is skipped with probability 0.15 (shared starts with different ends, and the converse); strand follows the gene with
    10 % flipped, 3 % carry 0x400, mapq is one of 0, 3, 30, 60.  The arrays are read-only and shared."""
    return _deck(seed)[0]


def junction_genes(seed=DECK_SEED):
    """the deck's genes as ranges (rid, loc, len, strand): first base of the first exon to last base of the last"""
    g = _deck(seed)[1]
    return dict(rid=np.asarray([x[0] for x in g], np.int32), loc=np.asarray([x[1] for x in g], np.int32),
                len=np.asarray([x[2] - x[1] + 1 for x in g], np.int32), strand=np.asarray([x[3] for x in g], np.int32))


def multiplicities(jr):
    """(the distinct (ref, start, end) as rows, their row counts)"""
    return np.unique(np.stack([jr["ref"], jr["start"], jr["end"]], axis=1), axis=0, return_counts=True)
