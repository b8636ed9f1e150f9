"""What bamCoverage(splice=True) must give, restated in numpy, and the decks both spliced suites use.

Semantics (the issue's, restated): walk a read's CIGAR with a cursor that starts at ``pos``.  ``M D = X`` (ops 0, 2, 7, 8)
advance it and are covered; ``N`` (op 3) advances it and is not; ``I S H P`` advance nothing.  A gap is a maximal stretch of
the read's span ``[pos, end]`` that comes from ``N`` operations; the read's blocks are the non-empty stretches between gaps.
A read with flag 0x4, or without a reference-consuming operation, keeps the single row ``[pos, pos]``; a read whose
reference-consuming operations are all ``N`` has no block.  Every block carries its read's flag, mapq and tlen.  The block
rows are stably sorted by (reference, block start): ties keep BAM order, then block order within the read.

Expected values of everything but tiny inputs: the existing oracle (``oracle_c.coverage_core``) applied to the block columns.
"""
from __future__ import annotations

import re

import numpy as np

OPS = "MIDNSHP=X"
_COVERED = (0, 2, 7, 8)


def cigar(text):
    """``"40M2000N60M"`` -> packed operations (``len << 4 | op``); ``"*"`` -> none."""
    if text == "*":
        return []
    return [int(n) << 4 | OPS.index(op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def _intervals(pos, flag, ops):
    """(covered pieces, gap pieces) of one read as lists of [start, end], pieces merged into maximal stretches; ``end``."""
    if flag & 0x4:
        return [[pos, pos]], [], pos
    cur, pieces = int(pos), []          # (kind, start, end), kind 1 covered, 0 gap
    for c in ops:
        op, ln = int(c) & 0xF, int(c) >> 4
        if ln == 0 or (op != 3 and op not in _COVERED):
            continue
        kind = 0 if op == 3 else 1
        if pieces and pieces[-1][0] == kind:
            pieces[-1][2] = cur + ln - 1
        else:
            pieces.append([kind, cur, cur + ln - 1])
        cur += ln
    if not pieces:
        return [[pos, pos]], [], pos
    return [p[1:] for p in pieces if p[0] == 1], [p[1:] for p in pieces if p[0] == 0], cur - 1


def _rid(cols):
    return np.repeat(np.arange(len(cols["ref_len"]), dtype=np.int32), np.diff(cols["ref_off"]))


def _rows(cols, which):
    """The rows (blocks: which = 0, gaps: which = 1) of all reads, stably sorted by (reference, start)."""
    rid = _rid(cols)
    coff, cig = cols["cigar_off"], cols["cigar"]
    r, s, e = [], [], []
    for i in range(len(cols["pos"])):
        got = _intervals(int(cols["pos"][i]), int(cols["flag"][i]), cig[coff[i]:coff[i + 1]])[which]
        for a, b in got:
            r.append(i); s.append(a); e.append(b)
    r = np.asarray(r, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    order = np.lexsort((s, rid[r])) if len(r) else np.zeros(0, dtype=np.int64)      # (lexsort is stable)
    r, s, e = r[order], s[order], np.asarray(e, dtype=np.int64)[order]
    n_ref = len(cols["ref_len"])
    return dict(ref_len=np.asarray(cols["ref_len"], dtype=np.int32),
                ref_off=np.searchsorted(rid[r], np.arange(n_ref + 1)).astype(np.int64),
                pos=s.astype(np.int32), end=e.astype(np.int32), flag=cols["flag"][r], mapq=cols["mapq"][r], tlen=cols["tlen"][r],
                read=r)


def blocks(cols):
    """Block columns (ref_len, ref_off, pos, end, flag, mapq, tlen, read) of CIGAR columns."""
    return _rows(cols, 0)


def gaps(cols):
    """The gap intervals as read columns carrying their read's flag, mapq and tlen."""
    return _rows(cols, 1)


def ends(cols):
    """bam_endpos - 1 of every read."""
    coff, cig = cols["cigar_off"], cols["cigar"]
    return np.asarray([_intervals(int(cols["pos"][i]), int(cols["flag"][i]), cig[coff[i]:coff[i + 1]])[2]
                       for i in range(len(cols["pos"]))], dtype=np.int32)


def brute_coverage(cols, rid, lo, hi, spliced):
    """Per-base coverage of [lo, hi) on reference ``rid``, one read and one base at a time (tiny inputs)."""
    out = np.zeros(hi - lo, dtype=np.int32)
    ref = _rid(cols)
    coff, cig = cols["cigar_off"], cols["cigar"]
    for i in np.flatnonzero(ref == rid):
        pos, flag = int(cols["pos"][i]), int(cols["flag"][i])
        if flag & 0x4:
            cover = [pos]
        else:
            cur, cover, any_ref = pos, [], False
            for c in cig[coff[i]:coff[i + 1]]:
                op, ln = int(c) & 0xF, int(c) >> 4
                if op in _COVERED or op == 3:
                    any_ref = any_ref or ln > 0
                    if op != 3 or not spliced:
                        cover.extend(range(max(cur, lo), min(cur + ln, hi)))
                    cur += ln
            if not any_ref:
                cover = [pos]
        for x in cover:
            if lo <= x < hi:
                out[x - lo] += 1
    return out


def columns(ref_len, reads):
    """reads: (rid, pos, flag, mapq, tlen, cigar text) in coordinate order -> CIGAR columns (with ``end``)."""
    ref_len = np.asarray(ref_len, dtype=np.int32)
    rid = np.asarray([r[0] for r in reads], dtype=np.int32)
    assert np.all(np.diff(rid.astype(np.int64) << 32 | (np.asarray([r[1] for r in reads], dtype=np.int64) + 1)) >= 0), "deck not sorted"
    ops = [cigar(r[5]) for r in reads]
    coff = np.concatenate([[0], np.cumsum([len(o) for o in ops])]).astype(np.int64)
    cols = dict(ref_len=ref_len, ref_off=np.searchsorted(rid, np.arange(len(ref_len) + 1)).astype(np.int64),
                pos=np.asarray([r[1] for r in reads], dtype=np.int32), flag=np.asarray([r[2] for r in reads], dtype=np.uint16),
                mapq=np.asarray([r[3] for r in reads], dtype=np.uint8), tlen=np.asarray([r[4] for r in reads], dtype=np.int32),
                cigar_off=coff, cigar=np.asarray([c for o in ops for c in o], dtype=np.uint32))
    cols["end"] = ends(cols)
    return cols


HAND_REF_LEN = [3_000_000, 5_000, 400_000]      # reference 1 stays empty between two used ones
LONG_OPS = 70_000                               # 1M1N repeated: more than a record's n_cigar_op holds


def hand_deck(with_pos_minus_one=True, with_long=True):
    """About 40 hand-written reads: every case the issue lists."""
    r0 = [
        (0, 100, 0, 30, 0, "100M"),
        (0, 150, 16, 40, 0, "40M2000N60M"),
        (0, 150, 0, 40, 0, "40M300N60M"),                       # same pos, another intron
        (0, 200, 0, 10, 0, "20M100N20M150N20M200N40M"),          # three N
        (0, 260, 16, 50, 0, "10M50N10M60N10M70N10M80N10M90N50M"),  # five N
        (0, 300, 0, 60, 0, "10N90M"),
        (0, 320, 16, 60, 0, "90M10N"),
        (0, 400, 0, 20, 0, "50M5N5N50M"),
        (0, 420, 0, 20, 0, "50M5N3I5N50M"),
        (0, 500, 16, 20, 0, "10S20M100N30M5H"),
        (0, 520, 0, 20, 0, "30M10D30M50N40M"),
        (0, 600, 0, 20, 0, "200N"),
        (0, 610, 0, 20, 0, "*"),
        (0, 620, 4, 20, 0, "50M100N50M"),
        (0, 700, 0x400, 5, 0, "40M2000N60M"),
        (0, 700, 16, 33, 150, "30M40N30M"),
        (0, 700, 0, 33, -150, "30M40N30M"),
        (0, 800, 0, 0, 0, "25M1N25M1N25M1N25M"),
        (0, 900, 16, 60, 0, "50=5X10N45M"),
        (0, 1000, 0, 60, 0, "10M0N90M"),
        (0, 1100, 0, 60, 0, "10M5N0M5N85M"),
        (0, 1200, 0, 60, 0, "3S10N4I90M2P10N"),
        (0, 2047, 16, 60, 0, "1M1N1M"),
        (0, 2048, 0, 60, 0, "1M4095N1M"),
        (0, 4000, 0, 60, 0, "100M"),
        (0, 1_000_000, 0, 60, 0, "50M1000000N50M"),              # an intron across hundreds of tiles
        (0, 1_000_010, 16, 7, 0, "50M1000000N50M"),
        (0, 1_500_000, 0, 60, 0, "100M"),
        (0, 2_000_030, 0, 60, 0, "100M"),
        (0, 2_999_900, 0, 60, 0, "50M200N50M"),                  # a gap past the reference's last base
        (0, 2_999_950, 16, 60, 0, "40M20N40M"),
    ]
    if with_pos_minus_one:
        r0 = [(0, -1, 0, 30, 0, "10M20N10M")] + r0
    r2 = [
        (2, 0, 0, 60, 0, "10M10N10M"),
        (2, 5, 16, 60, 0, "100M"),
        (2, 1000, 0, 60, 0, "40M2000N60M"),
        (2, 1000, 16, 60, 0, "40M1000N60M"),
        (2, 1020, 0, 60, 0, "100M"),
        (2, 399_000, 0, 60, 0, "100M500N100M"),
    ]
    if with_long:
        r2.insert(5, (2, 100_000, 0, 60, 0, "1M1N" * (LONG_OPS // 2)))
    return columns(HAND_REF_LEN, r0 + r2)


RANDOM_REF_LEN = [200_000, 200_000, 200_000]


def random_deck(n=5000, seed=20261020):
    """Seeded: n reads on three references of 200 kb with 0-5 introns of 1-50,000 bases each."""
    rng = np.random.default_rng(seed)
    g = np.sort(rng.integers(0, 600_000, n))
    rid, pos = (g // 200_000).astype(np.int32), (g % 200_000).astype(np.int32)
    n_intron = rng.integers(0, 6, n)
    ops, coff = [], [0]
    for k in n_intron:
        exons = rng.integers(1, 60, k + 1)
        introns = rng.integers(1, 50_001, k)
        for j in range(k + 1):
            ops.append(int(exons[j]) << 4 | 0)
            if j < k:
                ops.append(int(introns[j]) << 4 | 3)
        coff.append(len(ops))
    flag = np.where(rng.random(n) < 0.5, 16, 0).astype(np.uint16) | np.where(rng.random(n) < 0.03, 0x400, 0).astype(np.uint16)
    cols = dict(ref_len=np.asarray(RANDOM_REF_LEN, dtype=np.int32), ref_off=np.searchsorted(rid, np.arange(4)).astype(np.int64),
                pos=pos, flag=flag.astype(np.uint16), mapq=rng.integers(0, 61, n).astype(np.uint8),
                tlen=rng.integers(-500, 501, n).astype(np.int32), cigar_off=np.asarray(coff, dtype=np.int64),
                cigar=np.asarray(ops, dtype=np.uint32))
    cols["end"] = ends(cols)
    return cols


def spliced_prefix(cols, n):
    """The first n reads of ``cols`` that have an N: columns of their own (rows != reads)."""
    coff, cig = cols["cigar_off"], cols["cigar"]
    has_n = np.asarray([np.any((cig[coff[i]:coff[i + 1]] & 0xF) == 3) for i in range(len(cols["pos"]))])
    keep = np.flatnonzero(has_n)[:n]
    assert len(keep) == n
    return take(cols, keep)


def take(cols, keep):
    """The reads ``keep`` (ascending indices) as columns of their own."""
    coff, cig = cols["cigar_off"], cols["cigar"]
    rid = _rid(cols)[keep]
    lens = (coff[1:] - coff[:-1])[keep]
    new_cig = np.concatenate([cig[coff[i]:coff[i + 1]] for i in keep]) if len(keep) else np.zeros(0, dtype=np.uint32)
    out = dict(ref_len=cols["ref_len"], ref_off=np.searchsorted(rid, np.arange(len(cols["ref_len"]) + 1)).astype(np.int64),
               pos=cols["pos"][keep], flag=cols["flag"][keep], mapq=cols["mapq"][keep], tlen=cols["tlen"][keep],
               cigar_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), cigar=new_cig.astype(np.uint32))
    out["end"] = cols["end"][keep]
    return out


def n_share(cols):
    """(share of reads with an N, share with three or more) of CIGAR columns."""
    coff = cols["cigar_off"]
    is_n = np.concatenate([[0], np.cumsum((cols["cigar"] & 0xF) == 3)])
    per = is_n[coff[1:]] - is_n[coff[:-1]]
    return float(np.mean(per >= 1)), float(np.mean(per >= 3))


def oracle_reads(rows):
    from oracle import oracle_c
    return oracle_c.OracleReads(rows["ref_off"], rows["pos"], rows["end"], rows["flag"], rows["mapq"], rows["tlen"])


def expected_coverage(rows, rg, binsize=1, ss=False, **flt):
    """Coverage of the ranges by the rows (reads, blocks or gaps), flat in bsig_layout's order: the existing oracle per base,
    binned and split by strand here (a '-' range is mirrored first and binned second; sense = the range's strand, '*' = '+')."""
    from oracle import oracle_c
    rg = {k: np.asarray(v, dtype=np.int32) for k, v in rg.items()}
    if not ss:
        per, off = oracle_c.coverage_core(oracle_reads(rows), rg, **flt)
        parts = [per]
    else:
        parts = []
        for want_rev in (0, 16):
            sel = np.flatnonzero((rows["flag"] & 16) == want_rev)
            sub = dict(rows)
            rid = np.repeat(np.arange(len(rows["ref_len"])), np.diff(rows["ref_off"]))[sel]
            for k in ("pos", "end", "flag", "mapq", "tlen"):
                sub[k] = rows[k][sel]
            sub["ref_off"] = np.searchsorted(rid, np.arange(len(rows["ref_len"]) + 1)).astype(np.int64)
            per, off = oracle_c.coverage_core(oracle_reads(sub), rg, **flt)
            parts.append(per)
    out = []
    for i in range(len(rg["len"])):
        w = int(rg["len"][i])
        if w <= 0:
            continue
        cells = [np.add.reduceat(p[off[i]:off[i + 1]].astype(np.int64), np.arange(0, w, binsize)) for p in parts]
        if ss:
            fwd, rev = cells
            sense, anti = (rev, fwd) if rg["strand"][i] == -1 else (fwd, rev)
            out.append(np.stack([sense, anti], axis=1).reshape(-1))
        else:
            out.append(cells[0])
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, dtype=np.int32)
