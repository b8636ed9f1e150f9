"""The expected side of the strand cross-correlation tests (a helper, not a conftest): per range the oracle's per-base,
strand-split, unshifted pileup, then cross[d] = S[:w - d] . A[d:] and the moments in int64.  Never the GPU plan."""
import numpy as np


def oracle_reads(cols, mask=None):
    """columns (ref_off, pos, end, flag, mapq, tlen) -> the C oracle's reads"""
    from oracle import oracle_c
    if mask is None:
        return oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    ref_off = np.asarray(cols["ref_off"], dtype=np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    off = np.concatenate([[0], np.cumsum(np.bincount(rid[mask], minlength=len(ref_off) - 1))]).astype(np.int64)
    return oracle_c.OracleReads(off, cols["pos"][mask], cols["end"][mask], cols["flag"][mask], cols["mapq"][mask],
                                cols["tlen"][mask])


def np_reads(cols):
    """the same columns as the numpy oracle takes them (a reference id per read)"""
    ref_off = np.asarray(cols["ref_off"], dtype=np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    return dict(rid=rid, pos=np.asarray(cols["pos"], np.int64), end=np.asarray(cols["end"], np.int64),
                flag=np.asarray(cols["flag"], np.int64), mapq=np.asarray(cols["mapq"], np.int64),
                tlen=np.asarray(cols["tlen"], np.int64))


def rows(out, off, i):
    """sense and antisense rows (int64) of range i of a flat strand-split per-base result"""
    m = np.asarray(out[int(off[i]):int(off[i + 1])], dtype=np.int64).reshape(-1, 2)
    return m[:, 0], m[:, 1]


def from_rows(pairs, maxlag):
    """(S, A) per range -> (cross, moments), the definition"""
    cross = np.zeros(maxlag + 1, np.int64)
    mom = np.zeros(5, np.int64)
    for s, a in pairs:
        w = len(s)
        mom += np.asarray([w, s.sum(), a.sum(), (s * s).sum(), (a * a).sum()], np.int64)
        if w == 0:
            continue
        nz = np.flatnonzero(s)                    # (the sparse form of S[:w - d] . A[d:]: the same integers)
        sv = s[nz]
        for d in range(min(maxlag, w - 1) + 1):
            k = np.searchsorted(nz, w - d)
            cross[d] += int(np.dot(sv[:k], a[nz[:k] + d]))
    return cross, mom


def expected(cols, rg, maxlag, route="c", **kw):
    """cross (maxlag + 1) and moments (5) of the ranges rg over the reads cols; kw: the oracle's filter arguments
    (tlen_filter, mapqual, requiredF, filteredF).  route "c": oracle/oracle_c.py, "np": oracle/oracle_np.py"""
    n = len(rg["len"])
    if route == "c":
        from oracle import oracle_c
        out, off = oracle_c.pileup_core(cols if hasattr(cols, "c") else oracle_reads(cols), rg, binsize=1, shift=0, ss=True, **kw)
    else:
        from oracle import oracle_np
        out, off = oracle_np.pileup_core(np_reads(cols), rg, binsize=1, shift=0, ss=True, **kw)
    return from_rows((rows(out, off, i) for i in range(n)), maxlag)


def flat(cross, mom):
    return np.concatenate([cross, mom]).astype(np.int64)


def fragments(n_frag, length, ref_len, seed, read_len=40):
    """n_frag fragments of one length, each sequenced from both ends: a forward read at p, a reverse read ending at
    p + length - 1.  Returns unsorted columns (rid, pos, end, flag) on reference 0."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, ref_len - length - 1, n_frag).astype(np.int64)
    pos = np.concatenate([p, p + length - read_len])
    end = np.concatenate([p + read_len - 1, p + length - 1])
    flag = np.concatenate([np.zeros(n_frag, np.int64), np.full(n_frag, 16, np.int64)])
    return dict(rid=np.zeros(2 * n_frag, np.int64), pos=pos, end=end, flag=flag)


def merge_sorted(parts, n_ref):
    """unsorted (rid, pos, end, flag[, mapq, tlen]) column sets -> coordinate-sorted columns with ref_off"""
    cat = lambda k, d: np.concatenate([np.asarray(p[k]) if k in p else np.full(len(p["pos"]), d) for p in parts])  # noqa: E731
    rid, pos, end, flag = cat("rid", 0), cat("pos", 0), cat("end", 0), cat("flag", 0)
    mapq, tlen = cat("mapq", 60), cat("tlen", 0)
    o = np.lexsort((pos, rid))
    rid = rid[o]
    return dict(ref_off=np.searchsorted(rid, np.arange(n_ref + 1)).astype(np.int64), pos=pos[o].astype(np.int32),
                end=end[o].astype(np.int32), flag=flag[o].astype(np.uint16), mapq=mapq[o].astype(np.uint8),
                tlen=tlen[o].astype(np.int32))
