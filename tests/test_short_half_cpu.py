"""The 16-bit 5'-end columns of span classes 0 and 1 (bsig_types.h: p5h; BsigKParams::short_half), as a numpy model of
what k_make_short_p5h writes and what ProfileOne::half1 / oct read back, against the rule of bsig_plan_create:

    tile bases + 2 ext + 2 (maxspan - 1) + two buckets <= 2^15 - 256.

Encode: h = (5' end & 0x7FFF) | reverse << 15, 5' end = pos, or pos + span - 1 on the reverse strand.
Decode: 5' end = base + ((h - base) & 0x7FFF) with base the class's bucket-rounded window start of the tile
(ProfileOne::short_base), which is exact if and only if 0 <= 5' end - base < 2^15.

Inside the rule the largest distance a window can hold is (tile + 2 ext + maxspan - 1 + 2 buckets - 2 - 1) for pos
(rounding moves either end of the window by at most a bucket less one base) plus maxspan - 1 for a reverse read, so at
the rule's limit it is 2^15 - 256 - 3: the rule keeps the 256 bases the packed class's rule keeps (they cover a class-0
word whose 8-bit span field holds 255 for a span below 1) and the two bases of rounding.  The constant the decode
itself stands on is 2^15: at a distance of exactly 2^15 the half-word is that of the base itself."""
import numpy as np

POS_BITS = 15
MASK = (1 << POS_BITS) - 1


def encode(pos, span, rev):
    p5 = pos + np.where(rev, span - 1, 0)
    return ((p5 & MASK) | (rev.astype(np.int64) << POS_BITS)).astype(np.uint16)


def decode(h, base):
    h = h.astype(np.int64)
    return base + ((h - base) & MASK), (h >> POS_BITS).astype(bool)


def rule(tile, ext, maxspan, kshift):
    """bsig_plan_create's bound for one class"""
    return tile + 2 * ext + 2 * (maxspan - 1) + 2 * (1 << kshift) <= (1 << POS_BITS) - 256


def window(tlo, tile, ext, maxspan, kshift):
    """[base, rhi): the bucket-rounded positions a tile [tlo, tlo + tile) reads of a class (load_windows, short_base)"""
    wlo, whi = max(tlo - ext - maxspan + 1, 0), tlo + tile + ext
    return (wlo >> kshift) << kshift, (((whi - 1) >> kshift) + 1) << kshift


def test_decode_is_exact_inside_the_plans_bound():
    rng = np.random.default_rng(7)
    seen = 0
    while seen < 400:
        tile = int(rng.choice([64, 500, 1000, 2000, 2048, 8192]))
        ext = int(rng.choice([0, 75, 5000, 11000]))
        maxspan = int(rng.choice([1, 100, 256, 257, 2100, 4096]))
        kshift = int(rng.integers(4, 14))
        if not rule(tile, ext, maxspan, kshift):
            continue
        seen += 1
        tlo = int(rng.choice([0, 1, 4095, 4096, 70_000, (1 << 15) - 1, 1 << 15, (1 << 31) - (1 << 16)]))
        base, rhi = window(tlo, tile, ext, maxspan, kshift)
        assert rhi - base + maxspan - 1 <= (1 << POS_BITS) - 256 - 2
        n = 2000
        pos = rng.integers(base, rhi, n)
        pos[:4] = [base, base, rhi - 1, rhi - 1]                       # the window's two ends, ...
        span = rng.integers(1, maxspan + 1, n)
        span[:4] = [1, maxspan, 1, maxspan]                            # ... the shortest and the longest read, ...
        rev = rng.random(n) < 0.5
        rev[:4] = [False, True, False, True]                           # ... the far end on the reverse strand
        p5, strand = decode(encode(pos, span, rev), base)
        assert np.array_equal(p5, pos + np.where(rev, span - 1, 0)) and np.array_equal(strand, rev)


def test_the_spare_256_bases_cover_a_class_0_span_field_of_255():
    """Class 0 keeps span - 1 in 8 bits: a read whose end lies before its pos (span < 1) has 255 there, whatever the
    class's maxspan says; the pos + fm path counts its 5' end at pos + 255 and so must the column."""
    tile, ext, maxspan, kshift = (1 << POS_BITS) - 256 - 2 * 16, 0, 1, 4
    assert rule(tile, ext, maxspan, kshift) and not rule(tile + 1, ext, maxspan, kshift)
    base, rhi = window(16, tile, ext, maxspan, kshift)
    pos, span, rev = np.array([rhi - 1]), np.array([256]), np.array([True])
    p5, _ = decode(encode(pos, span, rev), base)
    assert p5[0] == rhi - 1 + 255 and p5[0] - base < 1 << POS_BITS


def test_one_base_beyond_the_decodes_reach_a_counterexample_exists():
    """The rule's constant is the 2^15 of the half-word: a 5' end 2^15 - 1 from the base comes back, one at 2^15 comes
    back as the base -- for every base, either strand."""
    for base in (0, 2048, 70_000, (1 << 31) - (1 << 16)):
        for rev in (False, True):
            span = np.array([4096 if rev else 1])
            far = base + MASK - (span - 1 if rev else 0)
            ok, _ = decode(encode(far, span, np.array([rev])), base)
            assert ok[0] == base + MASK
            bad, strand = decode(encode(far + 1, span, np.array([rev])), base)
            assert bad[0] == base != base + MASK + 1 and strand[0] == rev
