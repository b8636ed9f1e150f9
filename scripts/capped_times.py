#!/usr/bin/env python3
"""The capped plans (bsig_plan_run_capped, keepDup) timed on one GPU, in one process, each against the plain plan of the same
ranges and parameters -- code that keepDup did not touch.

Resident synthetic single-end-treated reads on one reference (bench.make_reads); a tiling of --ranges ranges of --width
bases, strands alternating.  Warm plans, HIP events over --steps after --warmup, a capped plan and its plain partner
alternated run by run; median, min and max in ms (the spread is max - min).  One JSON line per comparison:

  per_base   per-base strand-split profile, keepDup 1        against  Plan(PROFILE, binsize 1, ss)
  bins200    binsize-200 strand-split profile, keepDup 1     against  Plan(PROFILE, binsize 200, ss)
  count      strand-split count, keepDup 1                   against  Plan(COUNT, ss)
  coverage   coverage of the kept reads at L = --frag-len    against  Plan(COVERAGE_EX, frag_len)

Every line also says whether the capped plan with the largest cap (2^31 - 1) gave its plain partner's integers.

  python scripts/capped_times.py [--ref-len 250000000] [--ranges 50000] [--width 2000] [--frag-len 200] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=250_000_000)
    ap.add_argument("--density", type=float, default=0.2, help="reads a base (the north star: 5e8 reads on 2.5 Gbp)")
    ap.add_argument("--ranges", type=int, default=50_000)
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--frag-len", type=int, default=200)
    ap.add_argument("--keep-dup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import CappedPlan, Context, Plan, Reads, make_params

    ref_len = [a.ref_len]
    n_reads = int(a.density * a.ref_len) & ~1
    cols = bench.make_reads(n_reads, ref_len, a.seed, True)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    n = a.ranges
    step = max(a.width, a.ref_len // max(n, 1))
    rg = dict(rid=np.zeros(n, np.int32), loc=(step * np.arange(n)).astype(np.int32), len=np.full(n, a.width, np.int32),
              strand=np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int32))
    args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
    base = dict(ref_len=a.ref_len, reads=n_reads, n_ranges=n, width=a.width, keep_dup=a.keep_dup, steps=a.steps, warmup=a.warmup)

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

    cases = {
        "per_base": (make_params(_lib.MODE_PROFILE, binsize=1, ss=True), 0),
        "bins200": (make_params(_lib.MODE_PROFILE, binsize=200, ss=True), 0),
        "count": (make_params(_lib.MODE_COUNT, binsize=-1, ss=True), 0),
        "coverage": (make_params(_lib.MODE_COVERAGE_EX, binsize=1, ss=False), a.frag_len),
    }
    for name, (p, L) in cases.items():
        plain = Plan(*args, p, frag_len=L)
        capped = CappedPlan(*args, p, a.keep_dup, L)
        whole = CappedPlan(*args, p, 2 ** 31 - 1, L)
        assert plain.cells == capped.cells == whole.cells
        out = {k: torch.zeros(max(plain.cells, 4), dtype=torch.int32, device="cuda:0") for k in ("plain", "capped", "whole")}
        t = timed({"capped": lambda: capped.run_device(out["capped"].data_ptr()), "plain": lambda: plain.run_device(out["plain"].data_ptr())})
        whole.run_device(out["whole"].data_ptr())
        stream.synchronize()
        st, ps = capped.stats(), plain.stats()
        line = dict(base, what="resident step", case=name, frag_len=L, cells=plain.cells, ms=t,
                    capped_over_plain=round(t["capped"][0] / t["plain"][0], 3),
                    largest_cap_is_the_plain_plan=bool(torch.equal(out["whole"], out["plain"])),
                    kept=int(out["capped"].sum(dtype=torch.int64).item()), all=int(out["plain"].sum(dtype=torch.int64).item()),
                    tiles=st["n_items"], plain_tiles=ps["n_items"], runs=capped.runs, heavy_tiles=st["heavy_tiles"],
                    visits=st["visits"], plain_visits=ps["visits"], bytes_per_visit_packed=st["bytes_per_visit_packed"])
        print(json.dumps(line), flush=True)
        for q in (plain, capped, whole):
            q.close()
        del out
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
