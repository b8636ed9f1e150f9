#!/usr/bin/env python3
"""Resident sum over ranges (bsig_plan_run_sum) against the per-range step (bsig_plan_run) of the same ranges, in one
process on one GPU: the two steps alternate, each timed with HIP events over --steps after --warmup, as bench.py times
its step.  Prints one JSON line per shape: the median step of each, B_sum (the sum plan's algorithmic bytes) and the
fraction of 8 TB/s it reaches.

  python scripts/aggregate_times.py --steps 50 --warmup 5 [--shapes NS,COV,W10K,R200,C4] [--reads 5e8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REF_LEN = [250_000_000] * 10
SHAPES = {
    "NS": dict(ranges=100_000, width=2000, paired=False, mode="profile", args=dict(binsize=1)),
    "C4": dict(ranges=100_000, width=2000, paired=True, mode="profile",
               args=dict(binsize=1, ss=True, shift=75, pe_mid=True, requiredF=66, tlen_filter=(50, 500))),
    "COV": dict(ranges=100_000, width=2000, paired=False, mode="coverage", args=dict()),
    "W10K": dict(ranges=20_000, width=10_000, paired=False, mode="profile", args=dict(binsize=1)),
    "R200": dict(ranges=1_000_000, width=200, paired=False, mode="profile", args=dict(binsize=1)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="NS,COV,W10K,R200")
    ap.add_argument("--reads", type=float, default=5e8)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, Plan, Reads, SumPlan, make_params
    from bamsignals_amd.synth import synth_ranges

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()                 # (a stream of its own: the library launches on it, the events bracket it)
    ctx = Context(0, stream=stream.cuda_stream)
    loaded = {}
    for name in a.shapes.split(","):
        cfg = SHAPES[name]
        if cfg["paired"] not in loaded:
            loaded.clear()                       # (one read set in HBM at a time)
            cols = bench.make_reads(int(a.reads), REF_LEN, a.seed, cfg["paired"])
            loaded[cfg["paired"]] = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"],
                                          cols["tlen"], end=cols["end"])
            del cols
        reads = loaded[cfg["paired"]]
        rg = synth_ranges(cfg["ranges"], cfg["width"], REF_LEN, seed=a.seed + 1)
        mode = _lib.MODE_PROFILE if cfg["mode"] == "profile" else _lib.MODE_COVERAGE
        prm = make_params(mode, **cfg["args"])
        per = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], prm)
        agg = SumPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], prm)
        out = torch.empty(per.cells, dtype=torch.int32, device="cuda:0")
        tot = torch.empty(agg.cells, dtype=torch.int64, device="cuda:0")
        times = {"sum": [], "per_range": []}
        for k in range(a.warmup + a.steps):
            for key, fn in (("sum", lambda: agg.run_device(tot.data_ptr())), ("per_range", lambda: per.run_device(out.data_ptr()))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if k >= a.warmup:
                    times[key].append(e0.elapsed_time(e1))
        # the sum equals the per-range result summed in int64: every shape here has the same flat layout both ways
        stream.synchronize()
        want = out.cpu().numpy().reshape(cfg["ranges"], -1).sum(axis=0, dtype=np.int64)
        got = tot.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), name
        st_s, st_p = agg.stats(), per.stats()
        ms_s, ms_p = float(np.median(times["sum"])), float(np.median(times["per_range"]))
        print(json.dumps(dict(shape=name, desc=f"{cfg['ranges']} x {cfg['width']} {cfg['mode']} {cfg['args']}",
                              sum_ms=round(ms_s, 4), per_range_ms=round(ms_p, 4), ratio=round(ms_s / ms_p, 3),
                              B_sum_MB=round(st_s["algorithmic_bytes"] / 1e6, 1), B_MB=round(st_p["algorithmic_bytes"] / 1e6, 1),
                              sum_frac_of_8TBps=round(st_s["algorithmic_bytes"] / (ms_s * 1e-3) / 8e12, 3),
                              heavy_tiles=st_s["heavy_tiles"], exact=bool(np.array_equal(got, want)))),
              flush=True)
        per.close()
        agg.close()
        del out, tot


if __name__ == "__main__":
    main()
