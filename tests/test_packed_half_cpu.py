"""CPU: a numpy model of the packed class's 16-bit 5'-end column (bsig_types.h: p5h) and of how k_profile_half reads it
(kernels.hip: ProfileOne::oct), against the all-pairs int64 numpy oracle.  The model takes every tile's packed window as
the kernel does (bucket-rounded, one chunk from its start `base`), decodes d = (h - base) & 0x7FFF in 32-bit unsigned
arithmetic and places the read in the tile's cells.  Under bsig_plan_create's bound (tile bases + 2 ext + maxspan + two
buckets <= 2^15 - 256) it matches the oracle, reverse reads whose 5' end lies within 255 bases of the chunk's end
included; one window past the bound decodes some 5' ends a chunk short."""
import numpy as np

CHUNK = 1 << 15
UNIT = 16


def half_ok(tile_cells, ext, maxspan, kshift):
    """bsig_plan_create's window bound for the half form."""
    return tile_cells + 2 * ext + maxspan + 2 * (1 << kshift) <= CHUNK - 256


def encode(pos, end, rev):
    p5 = np.where(rev, end, pos).astype(np.int64)
    return ((p5 & 0x7FFF) | (rev.astype(np.int64) << 15)).astype(np.uint32)


def model_profile(cols, ranges, shift, ss, tile_cells, kshift, maxspan):
    """k_profile_half's result for bins of one base (no filter rejects a read), and the largest d it decoded."""
    rid, loc, ln, strand = (np.asarray(ranges[k]) for k in ("rid", "loc", "len", "strand"))
    S = 2 if ss else 1
    off = np.concatenate([[0], np.cumsum(ln.astype(np.int64) * S)])
    out = np.zeros(int(off[-1]), dtype=np.int64)
    ext = abs(shift)
    cd = np.uint32((-2 * shift) & 0xFFFFFFFF)
    d_max = 0
    ref_off = cols["ref_off"]
    for i in range(len(rid)):
        r = int(rid[i])
        lo_r, hi_r = int(ref_off[r]), int(ref_off[r + 1])
        pos, end = cols["pos"][lo_r:hi_r].astype(np.int64), cols["end"][lo_r:hi_r].astype(np.int64)
        rev = (cols["flag"][lo_r:hi_r] & 16) != 0
        h = encode(pos, end, rev)
        ref_bp = ((int(cols["ref_len"][r]) >> UNIT) + 1) << UNIT
        neg_range = strand[i] < 0
        L, lc0 = int(ln[i]), int(loc[i])
        for c0 in range(0, L, tile_cells):
            nc = min(tile_cells, L - c0)
            tlo, thi = (lc0 + L - c0 - nc, lc0 + L - c0) if neg_range else (lc0 + c0, lc0 + c0 + nc)
            wlo, whi = max(0, tlo - ext - maxspan + 1), min(ref_bp, thi + ext)
            if wlo >= whi:
                continue
            rlo = (wlo >> kshift) << kshift
            rhi = (((whi - 1) >> kshift) + 1) << kshift
            base = rlo
            sel = (pos >= rlo) & (pos < rhi)
            hs = h[sel]
            d = (hs - np.uint32(base)) & np.uint32(0x7FFF)
            if d.size:
                d_max = max(d_max, int(d.max()))
            nm = np.where((hs >> np.uint32(15)) & np.uint32(1), np.uint32(0xFFFFFFFF), np.uint32(0))
            fwd = d + (nm & cd)
            if neg_range:
                K = np.uint32((L - 1 - c0 - (base - lc0 + shift)) & 0xFFFFFFFF)
                lc = K - fwd
            else:
                K = np.uint32((base - lc0 + shift - c0) & 0xFFFFFFFF)
                lc = K + fwd
            ok = lc < np.uint32(nc)
            lc = lc[ok].astype(np.int64)
            if ss:
                anti = ((~nm if neg_range else nm) & np.uint32(1))[ok].astype(np.int64)
                cell = 2 * (c0 + lc) + anti
            else:
                cell = c0 + lc
            np.add.at(out, off[i] + cell, 1)
    return out, d_max


def _reads(seed):
    """Dense packed-class reads (spans 1..256, both strands) on three references, one of them short of a unit."""
    rng = np.random.default_rng(seed)
    ref_len = np.array([150_000, 70_000, 40_000], dtype=np.int32)
    n = [120_000, 60_000, 40_000]
    pos, end, flag, rid = [], [], [], []
    for r, k in enumerate(n):
        p = np.sort(rng.integers(0, ref_len[r], k))
        p[:3] = 0
        p[-3:] = ref_len[r] - 1                                   # reads at the reference's first and last base
        sp = np.where(rng.random(k) < 0.3, 256, rng.integers(1, 257, k))
        pos.append(p); end.append(p + sp - 1)
        flag.append(np.where(rng.random(k) < 0.5, 16, 0)); rid.append(np.full(k, r))
    cat = lambda x, t: np.concatenate(x).astype(t)
    cols = dict(ref_len=ref_len, pos=cat(pos, np.int32), end=cat(end, np.int32), flag=cat(flag, np.uint16),
                rid=cat(rid, np.int32))
    n_all = len(cols["pos"])
    cols["mapq"] = np.full(n_all, 30, dtype=np.uint8)
    cols["tlen"] = np.zeros(n_all, dtype=np.int32)
    cols["ref_off"] = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return cols


def _ranges(cols, width, n, seed):
    rng = np.random.default_rng(seed)
    rid = rng.integers(0, 3, n).astype(np.int32)
    loc = (rng.random(n) * (cols["ref_len"][rid] - width // 2)).astype(np.int32)
    loc[:3] = 0                                                   # ranges at reference starts ...
    loc[3:6] = cols["ref_len"][rid[3:6]] - width                  # ... ends ...
    loc[6:9] = cols["ref_len"][rid[6:9]] - width // 3             # ... and past them
    strand = rng.choice(np.array([1, -1, 0], dtype=np.int32), n)
    return dict(rid=rid, loc=loc, len=np.full(n, width, dtype=np.int32), strand=strand)


def _oracle(cols, rg, **a):
    from oracle import oracle_np
    reads = dict(rid=cols["rid"], pos=cols["pos"], end=cols["end"], flag=cols["flag"], mapq=cols["mapq"], tlen=cols["tlen"])
    want, _ = oracle_np.pileup_core(reads, rg, binsize=1, **a)
    return want


def test_half_word_model_matches_the_int64_oracle_up_to_the_window_bound():
    cols = _reads(7)
    maxspan = 256
    edge_hit = False
    for width, tile_cells in ((2000, 2000), (1000, 1000), (500, 500)):
        rg = _ranges(cols, width, 60, seed=width)
        for kshift in (4, 9):
            # the widest shift the bound allows, and a few well inside it
            ext_max = (CHUNK - 256 - tile_cells - maxspan - 2 * (1 << kshift)) // 2
            assert half_ok(tile_cells, ext_max, maxspan, kshift) and not half_ok(tile_cells, ext_max + 1, maxspan, kshift)
            for shift in (0, 75, -75, 5000, -5000, ext_max, -ext_max):
                for ss in (False, True):
                    got, d_max = model_profile(cols, rg, shift, ss, tile_cells, kshift, maxspan)
                    want = _oracle(cols, rg, shift=shift, ss=ss)
                    assert np.array_equal(got, want), (width, kshift, shift, ss, int(np.sum(got != want)))
                    assert d_max < CHUNK
                    edge_hit |= d_max >= CHUNK - 256
    # reverse reads whose 5' end lands within 255 bases of the chunk's end were decoded (and counted right)
    assert edge_hit


def test_half_word_model_breaks_past_the_bound():
    """The bound is not slack: a window 300 bases wider than it allows puts 5' ends a chunk past base, and the
    15-bit distance wraps."""
    cols = _reads(8)
    tile_cells, kshift, maxspan = 2000, 4, 256
    ext = (CHUNK - 256 - tile_cells - maxspan - 2 * (1 << kshift)) // 2 + 150
    rg = _ranges(cols, 2000, 60, seed=3)
    bad = 0
    for shift in (ext, -ext):
        got, _ = model_profile(cols, rg, shift, False, tile_cells, kshift, maxspan)
        bad += int(np.sum(got != _oracle(cols, rg, shift=shift)))
    assert bad > 0


def test_encoding_keeps_the_low_15_bits_and_the_strand():
    rng = np.random.default_rng(1)
    pos = rng.integers(0, 1 << 30, 100_000).astype(np.int64)
    end = pos + rng.integers(0, 256, pos.size)
    rev = rng.random(pos.size) < 0.5
    h = encode(pos, end, rev)
    assert h.max() < (1 << 16)
    assert np.array_equal((h >> 15) & 1, rev.astype(np.uint32))
    p5 = np.where(rev, end, pos)
    # any base at or below the 5' end within one chunk gives it back
    base = p5 - rng.integers(0, CHUNK, pos.size)
    d = (h.astype(np.int64) - base) & 0x7FFF
    assert np.array_equal(base + d, p5)
