"""CPU: the host-side parts of bench.py -- its threaded read generator against bamsignals_amd.synth, what
--dump-outputs writes, and the arguments a plain run refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench
from bamsignals_amd.synth import synth_reads


@pytest.mark.parametrize("threads", [1, 3, 8])
@pytest.mark.parametrize("ref_len", [[250_000, 0, 90_000, 1_000], [7_000_000]])
def test_threaded_reads_equal_the_generators(threads, ref_len):
    """The same columns, value for value and type for type, as synth_reads with the same seed."""
    for n in (0, 5, 100_003):
        want = synth_reads(n, ref_len, seed=0xBA51, paired=False, with_cigar=False)
        got = bench.synth_reads_threaded(n, ref_len, 0xBA51, threads)
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (n, k)


def test_paired_reads_come_from_the_generator():
    want = synth_reads(20_000, [300_000, 200_000], seed=7, paired=True, with_cigar=False)
    got = bench.make_reads(20_000, [300_000, 200_000], 7, True)
    assert all(np.array_equal(got[k], want[k]) for k in want)


class _Plan:
    def __init__(self, lens):
        self.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.cells = int(self.offsets[-1])


class _Workload:
    """What dump_outputs reads of a bench.Workload: the batches' plans and result buffers (padded past `cells`)."""
    def __init__(self, nb, lens, seed=3):
        import torch
        rng = np.random.default_rng(seed)
        self.nb = nb
        self.full_plans = [_Plan(lens) for _ in range(nb)]
        self.final = [torch.from_numpy(rng.integers(0, 1000, p.cells + 4).astype(np.int32)) for p in self.full_plans]


def test_dump_outputs_is_the_last_steps_result(tmp_path):
    lens = np.random.default_rng(1).integers(0, 50, 700)
    w = _Workload(3, lens)
    bench.dump_outputs(w, 5, str(tmp_path))           # steps 0..4 over 3 batches: the last one ran batch 1
    res = w.final[1].numpy()[:w.full_plans[1].cells].astype(np.int64)
    off = w.full_plans[1].offsets
    got = {k: np.load(tmp_path / (k + ".npy")) for k in ("cells_sample", "range_sums", "range_widths")}
    assert sorted(os.listdir(tmp_path)) == ["cells_sample.npy", "range_sums.npy", "range_widths.npy"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["cells_sample"], res)
    cs = np.concatenate([[0], np.cumsum(res)])
    assert np.array_equal(got["range_sums"], cs[off[1:]] - cs[off[:-1]])
    assert np.array_equal(got["range_widths"], np.diff(off))


def test_dump_outputs_samples_a_large_result_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CELLS", 1000)
    monkeypatch.setattr(bench, "DUMP_RANGES", 100)
    lens = np.full(5000, 7)
    w = _Workload(2, lens)
    for d in ("a", "b"):
        bench.dump_outputs(w, 2, str(tmp_path / d))
    for k in ("cells_sample", "range_sums", "range_widths"):
        x, y = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert np.array_equal(x, y) and 0 < x.size <= (1000 if k == "cells_sample" else 100)
    res = w.final[1].numpy()[:35000]
    sums = np.load(tmp_path / "a" / "range_sums.npy")
    assert set(sums.tolist()) <= set(res.reshape(-1, 7).sum(axis=1).astype(np.float64).tolist())


@pytest.mark.parametrize("args", [["--steps", "0"], ["--pipelined"], ["--strong"], ["--in-process-slots", "2"]])
def test_plain_run_refuses_what_only_full_measures(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 2 and "error:" in r.stderr, r.stderr


def test_a_dump_stays_under_64_mb():
    assert (bench.DUMP_CELLS + 2 * bench.DUMP_RANGES) * 8 <= 64e6
