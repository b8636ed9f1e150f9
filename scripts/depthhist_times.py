#!/usr/bin/env python3
"""Depth histogram (bsig_plan_run_hist) timed on one GPU, in one process.

Resident synthetic paired reads on one reference at each of --densities (reads a base: sparse and deep); two sets of
ranges, a tiling of the reference and --ranges one-kb ranges.  For each set, signal ("coverage"; "ends" with strands)
and row count (max_value = rows - 1) the resident step of a hist plan in its two forms -- BAMSIGNALS_HIST_FORM=plain:
one LDS atomic per cell; merge: the zero cells of a wave counted by ballot, the rows equal to the wave's first non-zero
lane's merged before the atomic -- each with its own tiles and with every tile forced onto the WIDE (32-bit image)
kernel (BAMSIGNALS_HEAVY_READS=4 when the plan is made), alternated with the yardstick: ONE run of the ordinary plan
of the same mode over the same reads and ranges, which reads the same bytes and also writes 4 bytes per cell.  HIP
events over --steps after --warmup; median, min and max in ms, and the ratios of the medians.  --piles: the same with
30 % of the reads moved into 1 % of the reference.

Prints one JSON line per measurement.

  python scripts/depthhist_times.py [--ref-len 250000000] [--densities 0.02,0.4] [--ranges 100000] [--steps 20]
                                    [--warmup 3] [--rows 101,1001,8192] [--piles]
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
    ap.add_argument("--densities", default="0.02,0.4", help="reads a base, sparse and deep (the north star: 0.2)")
    ap.add_argument("--ranges", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="101,1001,8192")
    ap.add_argument("--piles", action="store_true", help="30 %% of the reads in 1 %% of the reference")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, HistPlan, Plan, Reads, make_params
    from bamsignals_amd.synth import synth_ranges, tile_ranges

    ref_len = [a.ref_len]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    sets = {"tiling": tile_ranges(ref_len, 16384), "one_kb": synth_ranges(a.ranges, 1000, ref_len, seed=a.seed + 2)}

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

    for density in [float(x) for x in a.densities.split(",")]:
        n_reads = int(density * a.ref_len) & ~1
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
        reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
        base = dict(ref_len=a.ref_len, reads=n_reads, density=density, piles=bool(a.piles))
        for name, rg in sets.items():
            args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
            for signal in ("coverage", "ends"):
                prm = (lambda: make_params(_lib.MODE_COVERAGE)) if signal == "coverage" else \
                      (lambda: make_params(_lib.MODE_PROFILE, binsize=1, ss=True))
                op = Plan(*args, prm())
                oout = torch.empty(op.cells, dtype=torch.int32, device="cuda:0")
                for rows in [int(x) for x in a.rows.split(",")]:
                    plans = {}
                    for wide in (False, True):
                        for form in ("plain", "merge"):
                            os.environ["BAMSIGNALS_HIST_FORM"] = form
                            if wide:
                                os.environ["BAMSIGNALS_HEAVY_READS"] = "4"
                            plans[form + ("_wide" if wide else "")] = HistPlan(*args, prm(), rows - 1)
                            os.environ.pop("BAMSIGNALS_HEAVY_READS", None)
                    os.environ.pop("BAMSIGNALS_HIST_FORM")
                    res = {f: torch.zeros(rows + 2, dtype=torch.int64, device="cuda:0") for f in plans}
                    fns = {"ordinary": lambda: op.run_device(oout.data_ptr())}
                    for f in plans:
                        fns[f] = (lambda f=f: plans[f].run_device(res[f].data_ptr()))
                    t = timed(fns)
                    stream.synchronize()
                    # the same integers from every form, and the ordinary plan's cells agree with the moments
                    total = int(oout.to(torch.int64).sum().item())
                    same = all(bool(torch.equal(res[f], res["plain"])) for f in plans) and \
                        int(res["plain"][rows + 1].item()) == total and int(res["plain"][rows].item()) == op.cells
                    st = plans["plain"].stats()
                    line = dict(base, what="resident step", ranges=name, n_ranges=len(rg["rid"]), signal=signal, rows=rows,
                                ordinary_ms=t["ordinary"], **{f + "_ms": t[f] for f in plans},
                                **{f + "_over_ordinary": round(t[f][0] / t["ordinary"][0], 3) for f in plans},
                                merge_over_plain=round(t["merge"][0] / t["plain"][0], 3),
                                merge_over_plain_wide=round(t["merge_wide"][0] / t["plain_wide"][0], 3),
                                cells=op.cells, sum=total, forms_agree_with_the_ordinary_plan=same, tiles=st["n_items"],
                                runs=plans["plain"].runs, wide_tiles_when_forced=plans["plain_wide"].stats()["heavy_tiles"],
                                visits=st["visits"], B_hist_MB=round(st["algorithmic_bytes"] / 1e6, 1),
                                B_ordinary_MB=round(op.stats()["algorithmic_bytes"] / 1e6, 1))
                    print(json.dumps(line), flush=True)
                    for p in plans.values():
                        p.close()
                    del res
                op.close()
                del oout
        reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
