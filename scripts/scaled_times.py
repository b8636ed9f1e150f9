#!/usr/bin/env python3
"""Scaled regions (bsig_plan_run_scaled) timed on one GPU, in one process.

Resident synthetic single-end reads at the north star's density (0.2 reads a base) on one reference; four sets of ranges:
the north star's (--ranges ranges of 1 kb) cut into 10 and into 100 bins, a panel of --targets targets of 80 .. 400 bases
in 20 bins, and --genes "genes" of log-uniform widths 1 kb .. 100 kb in 100 bins (the wide-bin case: 10 .. 1,000 cells a
bin).  For each set and signal ("coverage"; "ends" with strands), warm, alternated step by step:

  (a) ScaledPlan.run_host()                        N int64 per range (and strand) come back; once with the plain consumer
                                                   and once with the segmented one (BAMSIGNALS_SCALED_SEGMENTED), and the
                                                   plan as made without that variable: the form its own rule picks
  (b) Plan.run_host() plus np.add.reduceat         the per-base result: 4 bytes per base over PCIe, then the bins summed
                                                   on the host
  (c) SummaryPlan.run_host(), no thresholds        the same walk with the cheapest per-range consumer

Wall-clock seconds of each call (median, min, max over --steps after --warmup; (b), seconds long, is called once and
reported as one number), and beside them the device time of (a) and (c) alone (HIP events around run_device).  (b)'s
result is compared with all three (a)s', integer for integer.

Prints one JSON line per measurement.

  python scripts/scaled_times.py [--ref-len 250000000] [--density 0.2] [--ranges 1000000] [--targets 50000] [--genes 20000]
                                 [--steps 7] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_bins(flat, off, S, N):
    """the bins from the per-base result on the host: (n, S, N) int64"""
    n = len(off) - 1
    out = np.zeros((n, S, N), np.int64)
    w = np.diff(off) // S
    if n and bool(np.all(w == w[0])) and w[0] >= N:             # ranges of one width: one reduceat for all of them
        w0 = int(w[0])
        edges = -(-np.arange(N, dtype=np.int64) * w0 // N)
        return np.add.reduceat(flat.reshape(n, w0, S), edges, axis=1, dtype=np.int64).transpose(0, 2, 1)
    for i in range(n):
        wi = int(w[i])
        if wi == 0:
            continue
        c = flat[off[i]:off[i + 1]].reshape(wi, S).T
        if wi >= N:                                               # (no bin is empty: the edges rise strictly)
            out[i] = np.add.reduceat(c, -(-np.arange(N, dtype=np.int64) * wi // N), axis=1, dtype=np.int64)
        else:
            np.add.at(out[i].T, np.arange(wi, dtype=np.int64) * N // wi, c.T)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=250_000_000)
    ap.add_argument("--density", type=float, default=0.2, help="reads a base (the north star: 0.2)")
    ap.add_argument("--ranges", type=int, default=1_000_000)
    ap.add_argument("--targets", type=int, default=50_000)
    ap.add_argument("--genes", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, Plan, Reads, ScaledPlan, SummaryPlan, make_params
    from bamsignals_amd.synth import synth_ranges

    ref_len = [a.ref_len]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    n_reads = int(a.density * a.ref_len) & ~1
    cols = bench.make_reads(n_reads, ref_len, a.seed, False)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    rng = np.random.default_rng(a.seed + 4)
    panel = synth_ranges(a.targets, 400, ref_len, seed=a.seed + 3)
    panel["len"] = rng.integers(80, 401, a.targets).astype(np.int32)
    genes = synth_ranges(a.genes, 100_000, ref_len, seed=a.seed + 5)
    genes["len"] = np.exp(rng.uniform(np.log(1000), np.log(100_000), a.genes)).astype(np.int32)
    one_kb = synth_ranges(a.ranges, 1000, ref_len, seed=a.seed + 2)
    sets = [("one_kb", one_kb, 10), ("one_kb", one_kb, 100), ("panel", panel, 20), ("genes", genes, 100)]

    def stats(v):
        return (round(float(np.median(v)), 5), round(min(v), 5), round(max(v), 5))

    for name, rg, N in sets:
        args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
        for signal in ("coverage", "ends"):
            ss = signal == "ends"
            S = 2 if ss else 1
            prm = (lambda: make_params(_lib.MODE_COVERAGE)) if signal == "coverage" else \
                  (lambda: make_params(_lib.MODE_PROFILE, binsize=1, ss=True))
            forms = {}
            for form, flag in (("plain", "0"), ("segmented", "1")):
                os.environ["BAMSIGNALS_SCALED_SEGMENTED"] = flag     # (read when the plan is made)
                forms[form] = ScaledPlan(*args, prm(), N)
            del os.environ["BAMSIGNALS_SCALED_SEGMENTED"]
            forms["default"] = ScaledPlan(*args, prm(), N)
            assert forms["plain"].segmented is False and forms["segmented"].segmented is True
            op, yp = Plan(*args, prm()), SummaryPlan(*args, prm(), ())
            off = np.asarray(op.offsets)
            res = {}

            def way(key, plan):
                def run():
                    res[key] = plan.run_host()
                return run

            def way_b():
                res["b"] = host_bins(op.run_host(), off, S, N)

            ways = [("plain", way("plain", forms["plain"])), ("segmented", way("segmented", forms["segmented"])),
                    ("default", way("default", forms["default"])), ("b", way_b), ("c", way("c", yp))]
            wall = {k: [] for k, _ in ways}
            for i in range(a.warmup + a.steps):
                for key, fn in ways:
                    if key == "b" and i != a.warmup:                # (seconds a call: one timed call says enough)
                        continue
                    stream.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    if i >= a.warmup:
                        wall[key].append(time.perf_counter() - t0)
            # the device time of the reductions alone
            da = torch.zeros(max(forms["plain"].cells, 1), dtype=torch.int64, device="cuda:0")
            dc = torch.zeros(max(yp.cells, 1), dtype=torch.int64, device="cuda:0")
            dev = {"plain": [], "segmented": [], "default": [], "c": []}
            for i in range(a.warmup + 3 * a.steps):
                for key, fn in (("plain", lambda: forms["plain"].run_device(da.data_ptr())),
                                ("segmented", lambda: forms["segmented"].run_device(da.data_ptr())),
                                ("default", lambda: forms["default"].run_device(da.data_ptr())),
                                ("c", lambda: yp.run_device(dc.data_ptr()))):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if i >= a.warmup:
                        dev[key].append(e0.elapsed_time(e1))
            st = forms["plain"].stats()
            med = {k: float(np.median(v)) for k, v in dev.items()}
            line = dict(ref_len=a.ref_len, reads=n_reads, ranges=name, n_ranges=len(rg["rid"]), n_bins=N, signal=signal,
                        a_plain_s=stats(wall["plain"]), a_segmented_s=stats(wall["segmented"]),
                        default_form="segmented" if forms["default"].segmented else "plain",
                        b_per_base_and_numpy_s=round(wall["b"][0], 5), c_summary_s=stats(wall["c"]),
                        a_plain_device_ms=stats(dev["plain"]), a_segmented_device_ms=stats(dev["segmented"]),
                        a_default_device_ms=stats(dev["default"]),
                        c_device_ms=stats(dev["c"]),
                        plain_over_c_device=round(med["plain"] / med["c"], 3),
                        segmented_over_plain_device=round(med["segmented"] / med["plain"], 3),
                        default_over_best_device=round(med["default"] / min(med["plain"], med["segmented"]), 3),
                        b_over_a=round(wall["b"][0] / float(np.median(wall["default"])), 1),
                        plain_equals_b=bool(np.array_equal(res["plain"], res["b"])),
                        segmented_equals_b=bool(np.array_equal(res["segmented"], res["b"])),
                        default_equals_b=bool(np.array_equal(res["default"], res["b"])),
                        a_sums_equal_c=bool(np.array_equal(res["plain"].sum(axis=2), res["c"][..., 0])),
                        result_bytes_a=int(res["plain"].nbytes), result_bytes_b=int(op.cells) * 4,
                        tiles=st["n_items"], runs=forms["plain"].runs, heavy_tiles=st["heavy_tiles"])
            print(json.dumps(line), flush=True)
            for p in (forms["plain"], forms["segmented"], forms["default"], op, yp):
                p.close()
            del da, dc
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
