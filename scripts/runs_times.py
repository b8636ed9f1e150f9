#!/usr/bin/env python3
"""Run-length coverage (bsig_runs_*, bamCoverage(runs=True)) timed on one GPU, in one process.

Single-end synthetic reads on one reference (--reads on --ref-len; "sparse": --sparse-reads on the same reference).
Shapes: the whole reference as one range, a tiling of 100,000 x 2 kb, 1,000,000 x 200 bp, and the whole reference over
the sparse reads.

(a) the encode step: bsig_runs_encode (count + scan + the read of the total + the allocation + emit + lengths) of a
    COVERAGE plan's result, alternated with the plan's own per-range step over the same ranges: HIP events over --steps
    after --warmup; median, min and max in ms.  B_runs = 8 B a cell (read twice) + 16 B a run (value and position
    written, position read, length written) + 16 B a segment; the achieved bytes/s of it beside the per-range kernel's
    (its algorithmic bytes over its time).
(b) the call: bamCoverage(runs=True) alternated with the only other route to the same answer, bamCoverage() and a numpy
    run-length encoder on the host, same process, same resident BAM, --calls each (wall seconds); the results are
    compared.  Only with --call (it writes the reads as a BAM into --workdir first).

Prints one JSON line per measurement.

  python scripts/runs_times.py [--ref-len 250000000] [--reads 50000000] [--sparse-reads 2000000] [--steps 20] [--warmup 3]
                               [--call] [--calls 3] [--workdir DIR] [--shapes whole,2kb,200bp,sparse]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_runs(sig):
    """the runs of a CountSignals' signals on the host, each range by itself: (seg_off, values, lengths)"""
    n = len(sig)
    flat = np.concatenate([np.asarray(s).reshape(-1) for s in sig]) if n else np.zeros(0, np.int32)
    cell0 = np.concatenate([[0], np.cumsum([s.size for s in sig])])
    start = np.ones(len(flat), bool)
    start[1:] = flat[1:] != flat[:-1]
    start[cell0[:-1][np.diff(cell0) > 0]] = True
    at = np.flatnonzero(start)
    return np.searchsorted(at, cell0, side="left"), flat[at], np.diff(np.concatenate([at, [len(flat)]])).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=250_000_000)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--sparse-reads", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--call", action="store_true", help="also (b): the file-level call against the host route")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--shapes", default="whole,2kb,200bp,sparse")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import GRanges, _lib, bamCoverage
    from bamsignals_amd.bamio import write_columns_as_bam
    from bamsignals_amd.device import Context, Plan, Reads, make_params
    from bamsignals_amd.synth import add_cigar, tile_ranges
    from bamsignals_amd.wrappers import last_call_route, last_call_timing

    ref_len = [a.ref_len]
    whole = dict(rid=np.zeros(1, np.int32), loc=np.zeros(1, np.int32), len=np.asarray(ref_len, np.int32), strand=np.ones(1, np.int32))

    def head(rg, n):
        return {k: v[:n] for k, v in rg.items()}
    shapes = {"whole": ("dense", whole), "2kb": ("dense", head(tile_ranges(ref_len, 2000), 100_000)),
              "200bp": ("dense", head(tile_ranges(ref_len, 200), 1_000_000)), "sparse": ("sparse", whole)}
    shapes = {k: v for k, v in shapes.items() if k in a.shapes.split(",")}
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()

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

    workdir = tempfile.mkdtemp(prefix="bsig_runs_times_", dir=a.workdir or os.environ.get("TMPDIR", "/tmp")) if a.call else None
    try:
        for data in ("dense", "sparse"):
            mine = {k: rg for k, (d, rg) in shapes.items() if d == data}
            if not mine:
                continue
            n_reads = a.reads if data == "dense" else a.sparse_reads
            cols = bench.make_reads(n_reads, ref_len, a.seed, False)
            base = dict(ref_len=a.ref_len, reads=n_reads)
            # ---- (a) the encode step beside the per-range step
            ctx = Context(0, stream=stream.cuda_stream)
            reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
            for name, rg in mine.items():
                plan = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_COVERAGE))
                out = torch.empty(plan.cells, dtype=torch.int32, device="cuda:0")
                enc = plan.runs()
                t = timed({"per_range": lambda: plan.run_device(out.data_ptr()), "encode": lambda: enc.encode(out.data_ptr())})
                stream.synchronize()
                st = plan.stats()
                b_runs = 8 * plan.cells + 16 * enc.n_runs + 16 * enc.n_seg
                print(json.dumps(dict(base, what="encode step", shape=name, n_ranges=len(rg["rid"]), cells=plan.cells, runs=enc.n_runs,
                                      per_range_ms=t["per_range"], encode_ms=t["encode"],
                                      encode_over_per_range=round(t["encode"][0] / t["per_range"][0], 3),
                                      B_runs_MB=round(b_runs / 1e6, 1), encode_GBps=round(b_runs / t["encode"][0] / 1e6, 1),
                                      B_per_range_MB=round(st["algorithmic_bytes"] / 1e6, 1),
                                      per_range_GBps=round(st["algorithmic_bytes"] / t["per_range"][0] / 1e6, 1),
                                      result_MB=dict(per_range=round(4 * plan.cells / 1e6, 1), runs=round((8 * enc.n_runs + 8 * enc.n_seg) / 1e6, 1)))),
                      flush=True)
                enc.close()
                plan.close()
                del out
            reads.close()
            ctx.close()
            if not a.call:
                continue
            # ---- (b) the call against the host route, on a resident BAM
            add_cigar(cols)
            bam = os.path.join(workdir, data + ".bam")
            write_columns_as_bam(bam, ["ref1"], cols, level=1)
            del cols
            os.environ["BAMSIGNALS_DECODE"] = "all"
            for name, rg in mine.items():
                gr = GRanges(["ref1"] * len(rg["rid"]), rg["loc"].astype(np.int64) + 1, width=rg["len"],
                             strand=[{1: "+", -1: "-", 0: "*"}[int(s)] for s in rg["strand"]])
                bamCoverage(bam, gr, runs=True, verbose=False)             # (the decode: not timed)
                t_new, t_old, parts, same = [], [], [], True
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    sig = bamCoverage(bam, gr, runs=True, verbose=False)
                    t_new.append(time.perf_counter() - t0)
                    lt = last_call_timing()
                    assert lt["bam_was_resident"] and "runs" in last_call_route()
                    parts.append((round(lt["plan"], 4), round(lt["kernels"], 4), round(lt["download"], 4)))
                    t0 = time.perf_counter()
                    plain = bamCoverage(bam, gr, verbose=False)
                    t1 = time.perf_counter()
                    old = host_runs(plain)
                    t_old.append((time.perf_counter() - t0, t1 - t0))
                    same = same and all(np.array_equal(x, y) for x, y in zip(old, (sig.seg_off, sig.values, sig.lengths)))
                    del plain, old
                new, oldt = np.asarray(t_new), np.asarray([x[0] for x in t_old])
                print(json.dumps(dict(base, what="call", shape=name, n_ranges=len(gr), calls=a.calls, runs=sig.nruns,
                                      runs_call_s=[round(float(np.median(new)), 4), round(float(new.min()), 4), round(float(new.max()), 4)],
                                      plan_kernels_download_s=parts,
                                      host_route_s=[round(float(np.median(oldt)), 4), round(float(oldt.min()), 4), round(float(oldt.max()), 4)],
                                      of_which_per_range_call_s=round(float(np.median([x[1] for x in t_old])), 4),
                                      host_over_runs=round(float(np.median(oldt) / np.median(new)), 2),
                                      faster_by_more_than_the_spread=bool(np.median(oldt) - np.median(new) > max(np.ptp(new), np.ptp(oldt))),
                                      same_result=bool(same))), flush=True)
            _lib.load().bsig_cache_clear()
    finally:
        if workdir:
            shutil.rmtree(workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
