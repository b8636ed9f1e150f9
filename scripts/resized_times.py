#!/usr/bin/env python3
"""bamCoverage's resident step on one GPU with and without reads resized to the fragment (Plan(frag_len=L)), in one process.

Resident synthetic single-end reads on one reference (--density reads a base), the reference tiled in 2-kb ranges.  Two
coverage plans over the same ranges, alternated inside one loop -- per-base coverage (k_coverage) and coverage in 50-bp
bins split by strand (k_coverage_bins) -- and, where the library has the resized creators, the same two with
frag_len = --frag-len, alternated in a loop of their own.  Then the forms deck (tests/forms_deck.py) at the same length, as a first data point of the resized
path on small, irregular ranges.  HIP events over --steps after --warmup; median, min and max in ms.

BSIG_LIB_PATH selects another build of the library (a parent commit's: only the plans it can make are timed, which says
whether this commit changed plain coverage's time).

Prints one JSON line per measurement.

  python scripts/resized_times.py [--ref-len 100000000] [--density 0.4] [--frag-len 200] [--steps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=100_000_000)
    ap.add_argument("--density", type=float, default=0.4)
    ap.add_argument("--frag-len", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()

    import torch

    import bench
    import forms_deck as deck
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, Plan, Reads, make_params
    from bamsignals_amd.synth import tile_ranges

    lib = _lib.load()
    resized = hasattr(lib, "bsig_plan_create_resized")           # (a parent commit's library: plain coverage alone)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    base = dict(library=os.path.relpath(_lib.SO_PATH, ROOT), frag_len=a.frag_len)

    def timed(fns):
        times = {k: [] for k in fns}
        for i in range(a.warmup + a.steps):
            for key, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    times[key].append(e0.elapsed_time(e1))
        return {k: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)) for k, v in times.items()}

    def measure(what, reads, rg, extra):
        args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
        kinds = {"cover": make_params(_lib.MODE_COVERAGE), "bins50_ss": make_params(_lib.MODE_COVERAGE_EX, binsize=50, ss=True)}
        plans = {k: Plan(*args, p) for k, p in kinds.items()}
        if resized:
            plans.update({k + "_resized": Plan(*args, p, frag_len=a.frag_len) for k, p in kinds.items()})
        outs = {k: torch.empty(max(p.cells, 4), dtype=torch.int32, device="cuda:0") for k, p in plans.items()}
        fns = {k: (lambda k=k: plans[k].run_device(outs[k].data_ptr())) for k in plans}
        # two loops: the plain pair alone, so that it alternates as it does under a library without the resized creators
        # (what else runs between two steps of a plan decides what they find in L2), then the resized pair
        t = timed({k: fns[k] for k in kinds})
        if resized:
            t.update(timed({k: f for k, f in fns.items() if k not in kinds}))
        st = {k: p.stats() for k, p in plans.items()}
        print(json.dumps(dict(base, what=what, n_ranges=len(rg["rid"]), **extra, **{k + "_ms": v for k, v in t.items()},
                              **{k + "_visits": s["visits"] for k, s in st.items()},
                              **{k + "_heavy_tiles": s["heavy_tiles"] for k, s in st.items()},
                              **{k + "_total": int(outs[k].to(torch.int64).sum().item()) for k in plans})), flush=True)
        for p in plans.values():
            p.close()

    ref_len = [a.ref_len]
    n_reads = int(a.density * a.ref_len) & ~1
    cols = bench.make_reads(n_reads, ref_len, a.seed, False)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    measure("resident step, 2-kb tiling", reads, tile_ranges(ref_len, 2000), dict(ref_len=a.ref_len, reads=n_reads))
    reads.close()
    c = deck.reads()
    reads = Reads(ctx, c["ref_len"], c["ref_off"], c["pos"], c["flag"], c["mapq"], c["tlen"], end=c["end"])
    measure("resident step, forms deck", reads, deck.ranges(), dict(reads=len(c["pos"])))
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
