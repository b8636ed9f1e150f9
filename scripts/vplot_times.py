#!/usr/bin/env python3
"""V-plot (bsig_plan_run_vplot) timed on one GPU, in one process.

Resident synthetic paired reads on one reference (the reads of scripts/fragsizes_times.py); --ranges ranges of --width bases,
tlen_filter (0, 1000), the midpoint rule.  Warm plans, HIP events over --steps after --warmup, the candidates of one table
alternated run by run; median, min and max in ms (the spread is max - min).  One JSON line per table:

  display   lenbin 5, binsize 10: 201 x 201 cells -- the plot as displayed
  full      lenbin 1, binsize 1: 1,001 x 2,001 cells -- the full-resolution plot
  small     lenbin 10, binsize 20: 101 x 101 cells -- a table inside the 64 KiB budget
  middle    lenbin 5, binsize 20: 201 x 101 cells -- a table between 64 KiB and the 160 KiB a workgroup may declare
  beyond    lenbin 2, binsize 10: 501 x 201 cells -- the first table past 160 KiB in this family

Candidates of a table: the form the plan chooses by itself (the LDS budget is all a workgroup may declare, 160 KiB), the
form it would choose at the 64 KiB the other reductions stop at (BAMSIGNALS_VPLOT_LDS_KIB=64), the global form
(BAMSIGNALS_VPLOT_FORM=global), and each of them with equal cells of a wave merged (BAMSIGNALS_VPLOT_MERGE=1); a candidate
that comes to the same kernel as the chosen one is left out.  All candidates of a table must give the same table.
Floors: one FragPlan run and one SumPlan run over the same ranges and filter -- the V-plot reads the same columns once, so
its distance from them is the cost of its atomics.
Yardstick: what a user does without the V-plot -- the loop of one SumPlan per row band on the same resident reads (display:
every band is planned and run; full: every --loop-stride-th band, scaled to all of them and said so).  The loop's rows
must be the V-plot's.

  python scripts/vplot_times.py [--ref-len 250000000] [--ranges 50000] [--width 2001] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = {"display": (5, 10), "full": (1, 1), "small": (10, 20), "middle": (5, 20), "beyond": (2, 10)}
KNOBS = ("BAMSIGNALS_VPLOT_FORM", "BAMSIGNALS_VPLOT_LDS_KIB", "BAMSIGNALS_VPLOT_MERGE")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=250_000_000)
    ap.add_argument("--density", type=float, default=0.2, help="reads a base (the north star: 5e8 reads on 2.5 Gbp)")
    ap.add_argument("--ranges", type=int, default=50_000)
    ap.add_argument("--width", type=int, default=2001)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tables", default="display,full,small,middle,beyond")
    ap.add_argument("--loop-stride", type=int, default=10, help="the full table's loop plans every n-th band")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, FragPlan, Reads, SumPlan, VplotPlan, make_params
    from bamsignals_amd.synth import synth_ranges

    ref_len = [a.ref_len]
    n_reads = int(a.density * a.ref_len) & ~1
    cols = bench.make_reads(n_reads, ref_len, a.seed, True)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    rg = synth_ranges(a.ranges, a.width, ref_len, seed=a.seed + 2)
    args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
    tf = (0, 1000)
    base = dict(ref_len=a.ref_len, reads=n_reads, n_ranges=a.ranges, width=a.width, tlen_filter=tf, rule="midpoint",
                steps=a.steps, warmup=a.warmup)

    def timed(fns, steps=a.steps, warmup=a.warmup):
        times = {k: [] for k in fns}
        for i in range(warmup + steps):
            for key, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i >= warmup:
                    times[key].append(e0.elapsed_time(e1))
        return {k: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)) for k, v in times.items()}

    def prof(binsize, band=tf):
        return make_params(_lib.MODE_PROFILE, tlen_filter=band, pe_mid=True, binsize=binsize, requiredF=66)

    def vplot(lenbin, binsize, **env):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        plan = VplotPlan(*args, prof(binsize), lenbin)
        for k in KNOBS:
            os.environ.pop(k, None)
        return plan

    for name in a.tables.split(","):
        lenbin, binsize = TABLES[name]
        cand = {"chosen": vplot(lenbin, binsize), "budget64": vplot(lenbin, binsize, BAMSIGNALS_VPLOT_LDS_KIB="64"),
                "global": vplot(lenbin, binsize, BAMSIGNALS_VPLOT_FORM="global")}
        merged = {"chosen+merge": vplot(lenbin, binsize, BAMSIGNALS_VPLOT_MERGE="1"),
                  "budget64+merge": vplot(lenbin, binsize, BAMSIGNALS_VPLOT_LDS_KIB="64", BAMSIGNALS_VPLOT_MERGE="1"),
                  "global+merge": vplot(lenbin, binsize, BAMSIGNALS_VPLOT_FORM="global", BAMSIGNALS_VPLOT_MERGE="1")}
        forms = {k: p.form for k, p in cand.items()}
        # (a candidate that is the same kernel as an earlier one is not timed twice)
        drop = [k for k, before in (("budget64", ("chosen",)), ("global", ("chosen", "budget64"))) if any(forms[k] == forms[b] for b in before)]
        for k in drop:
            cand.pop(k).close()
            merged.pop(k + "+merge").close()
        cand.update(merged)
        fp = FragPlan(*args, make_params(_lib.MODE_COUNT, tlen_filter=tf, pe_mid=True, binsize=-1, requiredF=66), lenbin)
        sp = SumPlan(*args, prof(binsize))
        rows, n_cols = cand["chosen"].rows, cand["chosen"].cols
        res = {k: torch.zeros(rows * n_cols, dtype=torch.int64, device="cuda:0") for k in cand}
        refused = {}
        for k in list(cand):        # (a launch the runtime refuses -- more LDS than it grants a workgroup -- is reported, not timed)
            try:
                cand[k].run_device(res[k].data_ptr())
                stream.synchronize()
            except _lib.BsigError as e:
                refused[k] = str(e)
                cand.pop(k).close()
                res.pop(k)
        fout = torch.zeros(fp.cells, dtype=torch.int64, device="cuda:0")
        sout = torch.zeros(sp.cells, dtype=torch.int64, device="cuda:0")
        fns = {k: (lambda k=k: cand[k].run_device(res[k].data_ptr())) for k in cand}
        fns["frag_floor"] = lambda: fp.run_device(fout.data_ptr())
        fns["sum_floor"] = lambda: sp.run_device(sout.data_ptr())
        t = timed(fns)
        stream.synchronize()
        table = res["chosen"].view(rows, n_cols)
        same = all(bool(torch.equal(res[k], res["chosen"])) for k in cand)
        marginals = bool(torch.equal(table.sum(dim=1), fout)) and bool(torch.equal(table.sum(dim=0), sout))
        st = cand["chosen"].stats()
        line = dict(base, what="resident step", table=name, lenbin=lenbin, binsize=binsize, rows=rows, cols=n_cols,
                    forms={k: ("global" if p.form else "lds") for k, p in cand.items()}, ms=t, fragments=int(table.sum().item()),
                    refused=refused, candidates_agree=same, marginals_are_the_floors=marginals, tiles=st["n_items"], runs=cand["chosen"].runs,
                    visits=st["visits"], chosen_over_frag_floor=round(t["chosen"][0] / t["frag_floor"][0], 3),
                    chosen_over_sum_floor=round(t["chosen"][0] / t["sum_floor"][0], 3))
        if name in ("display", "full"):
            # the yardstick: one SumPlan per row band, planned once, run in a loop
            stride = 1 if name == "display" else a.loop_stride
            bands = [(r, (r * lenbin, min(tf[1], (r + 1) * lenbin - 1))) for r in range(0, rows, stride)]
            loop = [(r, SumPlan(*args, prof(binsize, band))) for r, band in bands]
            lout = torch.zeros(len(loop), n_cols, dtype=torch.int64, device="cuda:0")
            tl = timed({"loop": lambda: [p.run_device(lout[i].data_ptr()) for i, (_, p) in enumerate(loop)]},
                       steps=max(3, a.steps // 4), warmup=1)
            stream.synchronize()
            idx = torch.tensor([r for r, _ in loop], device="cuda:0")
            line["loop_bands_run"] = len(loop)
            line["loop_ms"] = tl["loop"]
            line["loop_scaled_to_all_rows_ms"] = round(tl["loop"][0] * rows / len(loop), 3)
            line["loop_rows_are_the_vplots"] = bool(torch.equal(lout, table[idx]))
            line["loop_over_chosen"] = round(line["loop_scaled_to_all_rows_ms"] / t["chosen"][0], 1)
            for _, p in loop:
                p.close()
        print(json.dumps(line), flush=True)
        for p in list(cand.values()) + [fp, sp]:
            p.close()
        del res, fout, sout
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
