#!/usr/bin/env python3
"""Fragment-length histogram (bsig_plan_run_frag) timed on one GPU, in one process.

Resident synthetic paired reads on one reference; two sets of ranges, a tiling of the reference and --ranges one-kb
ranges.  For each set, rule ("filter" / "midpoint") and row count (101: tlen_filter (0, 1000) in rows of 10 lengths;
1,001: the same in rows of one; any other: tlen_filter (0, rows - 1) in rows of one) the resident
step of a frag plan in its two forms -- BAMSIGNALS_FRAG_FORM=plain: one LDS atomic per accepted read; merge: the rows
equal to the wave's first accepted lane's merged before the atomic -- alternated with the yardstick, ONE run of a COUNT
plan with the same tlen_filter over the same ranges (the same bytes per visit): HIP events over --steps after --warmup;
median, min and max in ms, and the ratios of the medians.  101 COUNT runs, one per row, are what a user pays today for
101 rows.  --piles: the same with 30 % of the reads moved into 1 % of the reference.

Prints one JSON line per measurement.

  python scripts/fragsizes_times.py [--ref-len 250000000] [--ranges 100000] [--steps 20] [--warmup 3] [--rows 101,1001,16384] [--piles]
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
    ap.add_argument("--ranges", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="101,1001,16384")
    ap.add_argument("--piles", action="store_true", help="30 %% of the reads in 1 %% of the reference")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, FragPlan, Plan, Reads, make_params
    from bamsignals_amd.synth import synth_ranges, tile_ranges

    ref_len = [a.ref_len]
    n_reads = int(a.density * a.ref_len) & ~1
    cols = bench.make_reads(n_reads, ref_len, a.seed, True)
    if a.piles:
        rng = np.random.default_rng(a.seed + 1)
        move = rng.random(n_reads) < 0.3
        pos = cols["pos"].astype(np.int64)
        span = cols["end"].astype(np.int64) - pos
        pos[move] = a.ref_len // 2 + rng.integers(0, a.ref_len // 100, int(move.sum()))
        o = np.argsort(pos, kind="stable")
        for k in ("flag", "mapq", "tlen"):
            cols[k] = np.ascontiguousarray(cols[k][o])
        cols["pos"] = pos[o].astype(np.int32)
        cols["end"] = (pos[o] + span[o]).astype(np.int32)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    sets = {"tiling": tile_ranges(ref_len, 16384), "one_kb": synth_ranges(a.ranges, 1000, ref_len, seed=a.seed + 2)}
    base = dict(ref_len=a.ref_len, reads=n_reads, piles=bool(a.piles))

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

    for name, rg in sets.items():
        for midpoint in (False, True):
            for rows in [int(x) for x in a.rows.split(",")]:
                tf, lenbin = ((0, 1000), 10) if rows == 101 else ((0, rows - 1), 1)
                args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
                cp = Plan(*args, make_params(_lib.MODE_COUNT, tlen_filter=tf, pe_mid=midpoint, binsize=-1, requiredF=66))
                cout = torch.empty(cp.cells, dtype=torch.int32, device="cuda:0")
                plans = {}
                for form in ("plain", "merge"):
                    os.environ["BAMSIGNALS_FRAG_FORM"] = form
                    plans[form] = FragPlan(*args, make_params(_lib.MODE_COUNT, tlen_filter=tf, pe_mid=midpoint, binsize=-1, requiredF=66), lenbin)
                os.environ.pop("BAMSIGNALS_FRAG_FORM")
                res = {f: torch.zeros(rows, dtype=torch.int64, device="cuda:0") for f in plans}
                t = timed({"count": lambda: cp.run_device(cout.data_ptr()),
                           "plain": lambda: plans["plain"].run_device(res["plain"].data_ptr()),
                           "merge": lambda: plans["merge"].run_device(res["merge"].data_ptr())})
                stream.synchronize()
                total = int(cout.to(torch.int64).sum().item())
                same = bool(torch.equal(res["plain"], res["merge"])) and int(res["merge"].sum().item()) == total
                st = plans["merge"].stats()
                line = dict(base, what="resident step", ranges=name, n_ranges=len(rg["rid"]), rule="midpoint" if midpoint else "filter",
                            rows=rows, count_ms=t["count"], plain_ms=t["plain"], merge_ms=t["merge"],
                            plain_over_count=round(t["plain"][0] / t["count"][0], 3), merge_over_count=round(t["merge"][0] / t["count"][0], 3),
                            merge_over_plain=round(t["merge"][0] / t["plain"][0], 3), fragments=total, rows_sum_to_the_count=same,
                            tiles=st["n_items"], runs=plans["merge"].runs, visits=st["visits"], B_frag_MB=round(st["algorithmic_bytes"] / 1e6, 1),
                            B_count_MB=round(cp.stats()["algorithmic_bytes"] / 1e6, 1))
                if rows == 101:
                    # what a user pays today for 101 rows: one COUNT run per length
                    per_len = [Plan(*args, make_params(_lib.MODE_COUNT, tlen_filter=(r * lenbin, r * lenbin + lenbin - 1), pe_mid=midpoint, binsize=-1, requiredF=66))
                               for r in range(0, rows, 25)]
                    tl = timed({"one": lambda: [p.run_device(cout.data_ptr()) for p in per_len]})
                    line["count_runs_for_101_rows_ms"] = round(tl["one"][0] / len(per_len) * rows, 3)
                    for p in per_len:
                        p.close()
                print(json.dumps(line), flush=True)
                for p in list(plans.values()) + [cp]:
                    p.close()
                del cout, res
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
