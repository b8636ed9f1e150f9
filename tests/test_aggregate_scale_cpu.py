"""CPU: the expected side of test_aggregate_scale_gpu.py.  On each of its inputs at a size the numpy oracle can take
(the forced-run grid as it is, the at-scale shapes with a twentieth of their ranges, the width groups of the extremes
at the first two shifts) the C oracle per range, summed in int64, equals the int64 numpy oracle per range, summed --
as test_oracle_extremes.py pins the per-range grid of test_parameter_extremes_gpu.py.

oracle_np holds every range against every read.  Here the ranges are taken in blocks in position order, each block
with the reads that can reach it (a window wider than shift, template length and the longest read together), which
leaves its arithmetic as it is and makes 4,100,000 reads affordable."""
import numpy as np
import pytest

import aggregate_scale_inputs as S
import extremes_inputs as X
from test_aggregate_cpu import _direct
from test_aggregate_scale_gpu import want_sum

READ_KEYS = ("rid", "pos", "end", "flag", "mapq", "tlen")


def np_sum(cols, rg, kind, b, ss, kw, block=64):
    """oracle_np per range, summed in int64, in the layout of want_sum"""
    pos, ref_off = np.asarray(cols["pos"], np.int64), np.asarray(cols["ref_off"], np.int64)
    reach = abs(kw.get("shift", 0)) + (kw["tlen_filter"][1] if kw.get("pe_mid") or kw.get("tspan") else 0)
    margin = reach + int((np.asarray(cols["end"], np.int64) - pos).max()) + 1
    order = np.lexsort((rg["loc"], rg["rid"]))
    tot = None
    for a in range(0, len(order), block):
        part = S.take(rg, order[a:a + block])
        near = []
        for r in np.unique(part["rid"]):
            sel = part["rid"] == r
            lo = int(part["loc"][sel].min()) - margin
            hi = int((part["loc"][sel].astype(np.int64) + part["len"][sel]).max()) + margin
            p = pos[ref_off[r]:ref_off[r + 1]]
            near.append(np.arange(ref_off[r] + np.searchsorted(p, lo), ref_off[r] + np.searchsorted(p, hi, side="right")))
        near = np.concatenate(near)
        reads = {k: np.asarray(cols[k])[near] for k in READ_KEYS}
        v = _direct(reads, part, b, "profile" if kind == "profile" else "coverage", ss, kw)
        tot = v if tot is None else tot + v
    return tot


def _same(cols, rg, cases):
    for kind, b, ss, kw in cases:
        want = want_sum(cols, rg, kind, b, ss, kw)
        got = np_sum(cols, rg, kind, b, ss, kw)
        assert want.dtype == np.int64 and got.shape == want.shape and want.any()
        assert np.array_equal(got, want), (kind, b, ss, kw)


@pytest.mark.parametrize("paired", [False, True])
def test_forced_run_grid(paired):
    cols = S.grid_reads(paired)
    for w in S.GRID_WIDTHS:
        _same(cols, S.grid_ranges(w), S.grid_cases(paired))


@pytest.fixture(scope="module")
def scale_cols():
    return S.scale_reads()


@pytest.mark.parametrize("n,w", S.SCALE_SHAPES, ids=lambda v: str(v))
def test_scale_shapes_at_a_twentieth(scale_cols, n, w):
    rg = S.scale_ranges(n // 20, w, seed=n)
    assert set(np.unique(rg["strand"])) == {-1, 0, 1}
    _same(scale_cols, rg, S.SCALE_CASES)


def test_extremes_width_groups():
    cols = X.make_reads()
    for shift in S.EXTREME_SHIFTS[:2]:
        rg, _ = X.place_ranges(X.REFS, X.CLUSTERS, shift)
        groups = S.width_groups(rg)
        assert set(groups) == set(X.WIDTHS)
        for idx in groups.values():
            _same(cols, S.take(rg, idx), [("profile", b, True, dict(shift=shift)) for b in (1, 50)])
    rg, _ = X.place_ranges(X.REFS, X.CLUSTERS, 8_000_000, hs=(0, 4_000_000))
    kw = dict(tspan=True, tlen_filter=X.COVERAGE_TF)
    for idx in S.width_groups(rg).values():
        _same(cols, S.take(rg, idx), [("cov2", 1, False, kw), ("covex", 50, True, kw)])
