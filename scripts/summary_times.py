#!/usr/bin/env python3
"""Per-range summaries (bsig_plan_run_summary) timed on one GPU, in one process.

Resident synthetic single-end reads at the north star's density (0.2 reads a base) on one reference; two sets of
ranges: the north star's (--ranges ranges of 1 kb) and a panel of --targets targets of 80 .. 400 bases.  For each set and
signal ("coverage"; "ends" with strands), warm, alternated step by step, three ways to the same integers:

  (a) SummaryPlan.run_host()                       3 + K int64 per range (and strand) come back
  (b) Plan.run_host() plus the numpy reductions    the parent's way: 4 bytes per base over PCIe, then sum / max / argmax /
                                                   count_nonzero per range on the host
  (c) HistPlan.run_host() on the same tiles        the same images built, one histogram kept

Wall-clock seconds of each call (median, min, max over --steps after --warmup), and beside them the device time of (a) and
(c) alone (HIP events around run_device), which is where the expectation "a is close to c" is tested.  (b)'s result is
compared with (a)'s, integer for integer.

Prints one JSON line per measurement.

  python scripts/summary_times.py [--ref-len 250000000] [--density 0.2] [--ranges 1000000] [--targets 50000]
                                  [--steps 7] [--warmup 2] [--thresholds 1,10,20,30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_reductions(flat, off, S, thresholds):
    """the parent's way from the per-base result: (n, S, 3 + K) int64"""
    n = len(off) - 1
    out = np.zeros((n, S, 3 + len(thresholds)), np.int64)
    w = np.diff(off) // S
    if n and bool(np.all(w == w[0])) and w[0] > 0:              # ranges of one width: one reshaped view, whole-array numpy
        c = flat.reshape(n, int(w[0]), S).transpose(0, 2, 1)
        out[..., 0] = c.sum(axis=2, dtype=np.int64)
        out[..., 1] = c.max(axis=2)
        out[..., 2] = c.argmax(axis=2)
        for k, t in enumerate(thresholds):
            out[..., 3 + k] = np.count_nonzero(c >= t, axis=2)
        return out
    for i in range(n):
        c = flat[off[i]:off[i + 1]].reshape(-1, S).T
        if c.shape[1] == 0:
            out[i, :, 2] = -1
            continue
        out[i, :, 0] = c.sum(axis=1, dtype=np.int64)
        out[i, :, 1] = c.max(axis=1)
        out[i, :, 2] = c.argmax(axis=1)
        for k, t in enumerate(thresholds):
            out[i, :, 3 + k] = np.count_nonzero(c >= t, axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=250_000_000)
    ap.add_argument("--density", type=float, default=0.2, help="reads a base (the north star: 0.2)")
    ap.add_argument("--ranges", type=int, default=1_000_000)
    ap.add_argument("--targets", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--thresholds", default="1,10,20,30")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, HistPlan, Plan, Reads, SummaryPlan, make_params
    from bamsignals_amd.synth import synth_ranges

    thr = tuple(int(x) for x in a.thresholds.split(",") if x)
    ref_len = [a.ref_len]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    n_reads = int(a.density * a.ref_len) & ~1
    cols = bench.make_reads(n_reads, ref_len, a.seed, False)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    panel = synth_ranges(a.targets, 400, ref_len, seed=a.seed + 3)
    panel["len"] = np.random.default_rng(a.seed + 4).integers(80, 401, a.targets).astype(np.int32)
    sets = {"one_kb": synth_ranges(a.ranges, 1000, ref_len, seed=a.seed + 2), "panel": panel}

    def stats(v):
        return (round(float(np.median(v)), 5), round(min(v), 5), round(max(v), 5))

    for name, rg in sets.items():
        args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
        for signal in ("coverage", "ends"):
            ss = signal == "ends"
            S = 2 if ss else 1
            prm = (lambda: make_params(_lib.MODE_COVERAGE)) if signal == "coverage" else \
                  (lambda: make_params(_lib.MODE_PROFILE, binsize=1, ss=True))
            sp, op, hp = SummaryPlan(*args, prm(), thr), Plan(*args, prm()), HistPlan(*args, prm(), 1000)
            off = np.asarray(op.offsets)
            res = {}

            def way_a():
                res["a"] = sp.run_host()

            def way_b():
                res["b"] = host_reductions(op.run_host(), off, S, thr)

            def way_c():
                res["c"] = hp.run_host()

            wall = {k: [] for k in "abc"}
            for i in range(a.warmup + a.steps):
                for key, fn in (("a", way_a), ("b", way_b), ("c", way_c)):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    if i >= a.warmup:
                        wall[key].append(time.perf_counter() - t0)
            # the device time of the two reductions alone
            da = torch.zeros(max(sp.cells, 1), dtype=torch.int64, device="cuda:0")
            dc = torch.zeros(hp.cells, dtype=torch.int64, device="cuda:0")
            dev = {"a": [], "c": []}
            for i in range(a.warmup + 3 * a.steps):
                for key, fn in (("a", lambda: sp.run_device(da.data_ptr())), ("c", lambda: hp.run_device(dc.data_ptr()))):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if i >= a.warmup:
                        dev[key].append(e0.elapsed_time(e1))
            st = sp.stats()
            line = dict(ref_len=a.ref_len, reads=n_reads, ranges=name, n_ranges=len(rg["rid"]), signal=signal, thresholds=thr,
                        a_summary_s=stats(wall["a"]), b_per_base_and_numpy_s=stats(wall["b"]), c_hist_s=stats(wall["c"]),
                        a_device_ms=stats(dev["a"]), c_device_ms=stats(dev["c"]),
                        a_over_c_device=round(float(np.median(dev["a"]) / np.median(dev["c"])), 3),
                        b_over_a=round(float(np.median(wall["b"]) / np.median(wall["a"])), 1),
                        a_equals_b=bool(np.array_equal(res["a"], res["b"])),
                        a_sum_equals_c_moment=int(res["a"][..., 0].sum()) == int(res["c"][-1]),
                        result_bytes_a=int(res["a"].nbytes), result_bytes_b=int(op.cells) * 4, result_bytes_c=int(res["c"].nbytes),
                        tiles=st["n_items"], runs=sp.runs, heavy_tiles=st["heavy_tiles"])
            print(json.dumps(line), flush=True)
            for p in (sp, op, hp):
                p.close()
            del da, dc
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
