"""CPU: the arithmetic the sum-over-ranges kernels follow (bsig_plan_create_sum), checked against the int64 numpy
oracle per range, then summed -- per-base tile images added up by tile position c0, for coverage a prefix sum that
restarts at every tile boundary, then bins in range orientation -- and the API's edges that need no GPU."""
import numpy as np
import pytest

from oracle import oracle_np


def _reads(seed, n=3000, ref_len=(40_000, 9_000)):
    rng = np.random.default_rng(seed)
    rid = np.sort(rng.integers(0, len(ref_len), n))
    pos = np.asarray([rng.integers(0, ref_len[r] - 300) for r in rid], np.int64)
    order = np.lexsort((pos, rid))
    rid, pos = rid[order], pos[order]
    span = rng.integers(1, 257, n)
    flag = np.where(rng.random(n) < 0.5, 16, 0) | np.where(rng.random(n) < 0.05, 1024, 0)
    tlen = rng.integers(-600, 600, n)
    return dict(rid=rid, pos=pos, end=pos + span - 1, flag=flag, mapq=rng.integers(0, 61, n), tlen=tlen), ref_len


def _ranges(n, w, ref_len, seed):
    rng = np.random.default_rng(seed)
    rid = rng.integers(0, len(ref_len), n)
    loc = np.asarray([rng.integers(0, max(ref_len[r] - w, 1)) for r in rid], np.int64)
    return dict(rid=rid, loc=loc, len=np.full(n, w, np.int64), strand=np.asarray([1, -1, 0])[rng.integers(0, 3, n)])


def _tile_image(reads, rg, i, c0, nc, mode, ss, kw):
    """one tile of one range, per base, as a kernel's image holds it (coverage: the tile's own difference image)"""
    one = {k: np.asarray(v)[i:i + 1] for k, v in rg.items()}
    if mode == "profile":
        out, _ = oracle_np.pileup_core(reads, one, binsize=1, ss=ss, **kw)
        S = 2 if ss else 1
        return out.astype(np.int64)[c0 * S:(c0 + nc) * S]
    if not ss:
        cov = oracle_np.coverage_core(reads, one, **kw)[0].astype(np.int64)
    else:
        fwd = (np.asarray(reads["flag"]) & 16) == 0
        sub = lambda m: {k: np.asarray(v)[m] for k, v in reads.items()}  # noqa: E731
        f = oracle_np.coverage_core(sub(fwd), one, **kw)[0].astype(np.int64)
        r = oracle_np.coverage_core(sub(~fwd), one, **kw)[0].astype(np.int64)
        sense, anti = (r, f) if one["strand"][0] < 0 else (f, r)
        cov = np.stack([sense, anti], axis=1).reshape(-1)
    S = 2 if ss else 1
    t = cov.reshape(-1, S)[c0:c0 + nc]
    d = t.copy()
    d[1:] -= t[:-1]                                   # self-contained: a tile's first cell holds its full value
    return d.reshape(-1)


def _model(reads, rg, w, tile, b, mode, ss, kw):
    S = 2 if ss else 1
    base = np.zeros(w * S, np.int64)
    for c0 in range(0, w, tile):                      # tiles of one c0 are summed together ...
        nc = min(tile, w - c0)
        acc = np.zeros(nc * S, np.int64)
        for i in range(len(rg["len"])):
            acc += _tile_image(reads, rg, i, c0, nc, mode, ss, kw)
        if mode == "coverage":                        # ... a scan that restarts at the tile boundary ...
            acc = np.cumsum(acc.reshape(nc, S), axis=0).reshape(-1)
        base[c0 * S:(c0 + nc) * S] = acc
    per = base.reshape(w, S)                          # ... then bins of the range-oriented bases
    binned = np.add.reduceat(per, np.arange(0, w, b), axis=0)
    return binned.T if ss else binned[:, 0]


def _direct(reads, rg, b, mode, ss, kw):
    n, w = len(rg["len"]), int(rg["len"][0])
    if mode == "profile":
        out, _ = oracle_np.pileup_core(reads, rg, binsize=b, ss=ss, **kw)
        s = out.astype(np.int64).reshape(n, -1).sum(axis=0)
        return s.reshape(-1, 2).T if ss else s
    sigs = []
    fwd = (np.asarray(reads["flag"]) & 16) == 0
    sub = lambda m: {k: np.asarray(v)[m] for k, v in reads.items()}  # noqa: E731
    allc = oracle_np.coverage_core(reads, rg, **kw)[0].astype(np.int64).reshape(n, w)
    if not ss:
        return np.add.reduceat(allc, np.arange(0, w, b), axis=1).sum(axis=0)
    f = oracle_np.coverage_core(sub(fwd), rg, **kw)[0].astype(np.int64).reshape(n, w)
    r = oracle_np.coverage_core(sub(~fwd), rg, **kw)[0].astype(np.int64).reshape(n, w)
    neg = (np.asarray(rg["strand"]) < 0)[:, None]
    for row in (np.where(neg, r, f), np.where(neg, f, r)):
        sigs.append(np.add.reduceat(row, np.arange(0, w, b), axis=1).sum(axis=0))
    return np.stack(sigs)


@pytest.mark.parametrize("mode", ["profile", "coverage"])
@pytest.mark.parametrize("w,tile,b", [(64, 64, 1), (100, 32, 7), (130, 64, 50), (257, 64, 13), (33, 8, 33)])
@pytest.mark.parametrize("ss", [False, True])
def test_decomposition_matches_the_oracle(mode, w, tile, b, ss):
    reads, ref_len = _reads(seed=w + tile)
    rg = _ranges(12, w, ref_len, seed=b)
    kw = dict(shift=40, mapqual=5, filteredF=1024) if mode == "profile" else dict(mapqual=5, filteredF=1024)
    assert np.any(rg["strand"] < 0)
    want = _direct(reads, rg, b, mode, ss, kw)
    got = _model(reads, rg, w, tile, b, mode, ss, kw)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_exactness_bound():
    """the flush bound of k_sum_tiles: 65,536 tiles of an unsliced image fit 32 bits (unsigned / signed)"""
    assert 65_536 * 32_768 <= 2 ** 32 - 1
    assert 65_536 * 32_767 < 2 ** 31


def test_unequal_widths_fail_before_any_native_call():
    from bamsignals_amd import GRanges, bamCoverage, bamProfile
    gr = GRanges(["chr1", "chr1"], [1, 100], width=[10, 11], strand=["+", "-"])
    for fn in (bamProfile, bamCoverage):
        with pytest.raises(ValueError, match="all signals must have the same length"):
            fn("/nonexistent/file.bam", gr, verbose=False, aggregate=True)


def test_bamcount_has_no_aggregate():
    from bamsignals_amd import GRanges, bamCount
    gr = GRanges(["chr1"], [1], width=[10], strand=["+"])
    with pytest.raises(TypeError):
        bamCount("/nonexistent/file.bam", gr, verbose=False, aggregate=True)
