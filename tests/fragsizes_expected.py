"""The expected side of the fragment-length histogram tests (a helper, not a conftest): the definition, literally -- per
row one bamCount of the C oracle with the row's band of lengths as its tlen filter, summed over the ranges.  Never the
GPU plan.  `restated` is the same thing said directly in numpy (filter, position, bincount), for the CPU tests."""
import numpy as np

from crosscorr_expected import merge_sorted, oracle_reads  # noqa: F401  (shared column helpers)


def n_rows(tf, lenbin):
    return int(tf[1]) // int(lenbin) + 1


def expected(cols, rg, tf, lenbin, midpoint, **filters):
    """hist[r] = sum_i bamCount(rg[i], shift 0, unstranded, requiredF 66, pe_mid = midpoint, tlen_filter = row r's band);
    filters: the oracle's mapqual / filteredF.  cols: columns or the oracle's reads."""
    from oracle import oracle_c
    orc = cols if hasattr(cols, "c") else oracle_reads(cols)
    hist = np.zeros(n_rows(tf, lenbin), np.int64)
    if len(rg["len"]) == 0:
        return hist
    for r in range(len(hist)):
        band = (max(int(tf[0]), r * lenbin), min(int(tf[1]), (r + 1) * lenbin - 1))
        if band[0] > band[1]:
            continue
        out, _ = oracle_c.pileup_core(orc, rg, binsize=-1, shift=0, ss=False, requiredF=66, pe_mid=bool(midpoint),
                                      tlen_filter=band, **filters)
        hist[r] = int(np.asarray(out, np.int64).sum())
    return hist


def whole_count(cols, rg, tf, midpoint, **filters):
    """the oracle's one bamCount with the whole filter, summed over the ranges"""
    from oracle import oracle_c
    orc = cols if hasattr(cols, "c") else oracle_reads(cols)
    if len(rg["len"]) == 0:
        return 0
    out, _ = oracle_c.pileup_core(orc, rg, binsize=-1, shift=0, ss=False, requiredF=66, pe_mid=bool(midpoint),
                                  tlen_filter=tuple(int(x) for x in tf), **filters)
    return int(np.asarray(out, np.int64).sum())


def restated(cols, rg, tf, lenbin, midpoint, mapqual=0, filteredF=-1):
    """filter, position, bincount(a // lenbin) per range (read_rejected: oracle/bamsignals_oracle.c:91-102)"""
    ref_off = np.asarray(cols["ref_off"], np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    pos, end = np.asarray(cols["pos"], np.int64), np.asarray(cols["end"], np.int64)
    flag, mapq = np.asarray(cols["flag"], np.int64), np.asarray(cols["mapq"], np.int64)
    a = np.abs(np.asarray(cols["tlen"], np.int64))
    nf = ~flag
    ok = (mapq >= mapqual) & ((66 & nf) == 0) & ((np.int64(filteredF) & nf & 0xFFFFFFFF) != 0) & (a >= tf[0]) & (a <= tf[1])
    neg = (flag & 16) != 0
    off = a // 2 if midpoint else 0
    p5 = np.where(neg, end - off, pos + off)
    hist = np.zeros(n_rows(tf, lenbin), np.int64)
    for r, lo, w in zip(rg["rid"], rg["loc"], rg["len"]):
        m = ok & (rid == r) & (p5 >= lo) & (p5 < int(lo) + int(w))
        hist += np.bincount(a[m] // lenbin, minlength=len(hist)).astype(np.int64)
    return hist


def planted(n, length, at, rid=0, reverse=False, read_len=40, mapq=60, negative_tlen=False, extra_flag=0):
    """n first-of-pair reads of fragments of one length with their 5' end on base `at` (unsorted columns): a forward
    read starts there (flag 99, tlen +length); a reverse read ENDS there (flag 83, tlen -length)"""
    at = np.broadcast_to(np.asarray(at, np.int64), (n,)).copy()
    pos = at - (read_len - 1) if reverse else at
    tl = -length if (reverse != negative_tlen) else length
    return dict(rid=np.full(n, rid, np.int64), pos=pos, end=pos + read_len - 1,
                flag=np.full(n, (83 if reverse else 99) | extra_flag, np.int64), mapq=np.full(n, mapq, np.int64),
                tlen=np.full(n, tl, np.int64))
