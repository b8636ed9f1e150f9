"""Inputs shared by test_aggregate_scale_gpu.py and test_aggregate_scale_cpu.py: the reads, ranges and parameter sets
on which sums over ranges (bsig_plan_create_sum) are held against the oracle with many tiles per wave.

Three inputs: the forced-run grid (the reads of test_aggregate_gpu.py, 600 ranges of each of three widths, the run
length of a sum plan forced through BAMSIGNALS_SUM_RUN_TILES); the sizes sum plans were built for (4,000,000 paired
reads and a pile of 100,000 on one locus, 30,000 to 300,000 ranges); and the groups of one width of the ranges that
extremes_inputs.place_ranges puts where megabase shifts and template lengths move the reads.

A case is (kind, binsize, ss, oracle keywords): kind "profile" (bamProfile), "cov2" (bamCoverage per base, mode 2) or
"covex" (bamCoverage in bins / by strand).
"""
import numpy as np

import extremes_inputs as X

# ---- the forced-run grid -------------------------------------------------------------------------------------------
GRID_REF = [2_000_000, 700_017]
GRID_WIDTHS = (100, 2_049, 10_000)
GRID_RANGES = 600
# 1 is below the waves of a workgroup (idle waves); 3 and 5 do not divide by them (the waves of one run take different
# numbers of tiles); 1,000 holds all 600 tiles of a tile position in one run
RUN_TILES = (1, 2, 3, 5, 64, 1_000)
THREADS = (64, 128, 256)
TILE_CELLS = (64, 68, 1_000, 4_096)
PE_ARGS = dict(tlen_filter=(50, 500), requiredF=66)       # first mates of proper pairs, as flagMask("midpoint") / ("extend")


def grid_reads(paired):
    """the reads of test_aggregate_gpu.py's `synth` fixture"""
    from bamsignals_amd.synth import synth_reads
    from oracle import oracle_c
    cols = synth_reads(400_000, GRID_REF, seed=91 + paired, paired=paired)
    cols["end"] = oracle_c.cigar_end(cols["pos"], cols["flag"], cols["cigar_off"], cols["cigar"])
    return cols


def grid_ranges(w):
    from bamsignals_amd.synth import synth_ranges
    rg = synth_ranges(GRID_RANGES, w, GRID_REF, seed=4_000 + w)
    assert set(np.unique(rg["strand"])) == {-1, 0, 1}
    return rg


def grid_cases(paired):
    if not paired:
        out = [("profile", b, ss, {}) for ss in (False, True) for b in (1, 7)]
        return out + [("cov2", 1, False, {}), ("covex", 1, True, {}), ("covex", 50, True, {})]
    mid = dict(PE_ARGS, pe_mid=True, shift=75)
    ext = dict(PE_ARGS, tspan=True)
    out = [("profile", b, ss, mid) for ss in (False, True) for b in (1, 7)]
    return out + [("cov2", 1, False, ext), ("covex", 1, True, ext), ("covex", 50, True, ext)]


# ---- the sizes sum plans were built for ----------------------------------------------------------------------------
SCALE_REF = [6_000_000, 2_000_017]
SCALE_READS = 4_000_000
SCALE_SHAPES = ((300_000, 200), (60_000, 2_049), (30_000, 10_000))
PILE_AT, PILE_W, PILE_READS = 3_000_000, 300, 100_000      # on reference 0
SCALE_CASES = (("profile", 1, False, dict(PE_ARGS, pe_mid=True, shift=75)),
               ("profile", 1, True, dict(PE_ARGS, pe_mid=True, shift=75)),
               ("cov2", 1, False, dict(PE_ARGS, tspan=True)),
               ("covex", 50, True, dict(PE_ARGS, tspan=True)))


def add_pile(cols, rid, at, width, n, seed):
    """`cols` with n more reads of 40 bases starting within `width` bases of `at` on reference `rid`: both strands, all
    first mates of proper pairs with template lengths of 100-400"""
    rng = np.random.default_rng(seed)
    pos = (at + rng.integers(0, width, n)).astype(np.int32)
    fwd = rng.random(n) < 0.5
    extra = dict(rid=np.full(n, rid, np.int32), pos=pos, end=pos + 39, flag=np.where(fwd, 99, 83).astype(np.uint16),
                 mapq=np.full(n, 60, np.uint8), tlen=(np.where(fwd, 1, -1) * rng.integers(100, 401, n)).astype(np.int32))
    out = {k: np.concatenate([np.asarray(cols[k]), extra[k]]) for k in extra}
    order = np.lexsort((out["pos"], out["rid"]))
    out = {k: v[order] for k, v in out.items()}
    n_ref = len(cols["ref_len"])
    out["ref_len"] = np.asarray(cols["ref_len"])
    out["ref_off"] = np.concatenate([[0], np.cumsum(np.bincount(out["rid"], minlength=n_ref))]).astype(np.int64)
    return out


def scale_reads(n=SCALE_READS, pile=PILE_READS):
    from bamsignals_amd.synth import synth_reads
    cols = synth_reads(n, SCALE_REF, seed=3, paired=True, with_cigar=False)
    return add_pile(cols, 0, PILE_AT, PILE_W, pile, seed=4)


def scale_ranges(n, w, seed=None):
    """n ranges of width w, all three strands; one in 64 of them (more than 1 %) overlaps the pile"""
    from bamsignals_amd.synth import synth_ranges
    rg = synth_ranges(n, w, SCALE_REF, seed=n if seed is None else seed)
    rng = np.random.default_rng(w)
    over = np.arange(0, n, 64)
    rg["rid"][over] = 0
    rg["loc"][over] = PILE_AT + PILE_W // 2 - rng.integers(0, w, len(over))
    assert len(over) * 100 >= n and set(np.unique(rg["strand"][over])) == {-1, 0, 1}
    return rg


# ---- groups of one width on the extremes inputs --------------------------------------------------------------------
EXTREME_SHIFTS = (0, 4_194_305, -5_000_000, 2**23, -20_000_000)
EXTREME_MIDPOINT = ((0, (0, 1_000_000_000)), (4_177_000, (0, 2**30 - 4_177_000)))
assert all(m in X.MIDPOINT for m in EXTREME_MIDPOINT) and all(s in X.SHIFTS for s in EXTREME_SHIFTS)


def width_groups(rg):
    """{width: indices} of the ranges by their actual width (a range narrowed by a short reference goes to the group
    of the width it has), groups of fewer than 2 ranges left out; at least 90 % of the ranges must remain"""
    out = {}
    for w in np.unique(rg["len"]):
        idx = np.flatnonzero(rg["len"] == w)
        if len(idx) >= 2:
            out[int(w)] = idx
    assert sum(len(v) for v in out.values()) * 10 >= 9 * len(rg["len"]), "fewer than 90 % of the placed ranges kept"
    return out


def take(rg, idx):
    return {k: np.asarray(v)[idx] for k, v in rg.items()}
