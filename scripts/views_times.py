#!/usr/bin/env python3
"""The views encoder (bsig_views_encode) timed beside the runs encoder (bsig_runs_encode) on the same device buffers, on
one GPU, in one process.

Buffers: (a) the per-base coverage of two whole references (2,000,000 and 700,017 bases; 400,000 synthetic paired reads,
seed 92) as a COVERAGE plan wrote it; (b) a synthetic buffer of --cells int32 (default 2^28) in four segments: values
0 .. 39 that change every 32 cells on average.  `lower` is the smallest value at most one cell in ten reaches.

Both encodes synchronise, so a host clock around the call is the time of count + scan + the read of the total + the
allocation + emit (+ lengths / unpack).  The two encoders alternate, --steps timed after --warmup; median, min and max in
ms, and the bytes the encoder's byte model asks for over the median.  Prints one JSON line per measurement.

  python scripts/views_times.py [--cells 268435456] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    n = fn()
    return (time.perf_counter() - t0) * 1e3, n


def measure(name, ctx, views, runs, ptr, cells, n_seg, lower, steps, warmup):
    tv, tr = [], []
    for k in range(warmup + steps):
        a, nv = timed(lambda: views.encode(ptr, lower))
        b, nr = timed(lambda: runs.encode(ptr))
        if k >= warmup:
            tv.append(a)
            tr.append(b)
    for what, t, n, per in (("views", tv, nv, 24 + 16), ("runs", tr, nr, 16)):
        model = 8 * cells + per * n + 16 * n_seg
        print(json.dumps(dict(buffer=name, encoder=what, cells=cells, segments=n_seg, lower=lower if what == "views" else None,
                              results=n, ms_median=round(float(np.median(t)), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                              model_bytes=model, model_GBps=round(model / np.median(t) / 1e6, 1), steps=steps)), flush=True)


def decile(flat):
    counts = np.bincount(np.clip(flat, 0, 1 << 16))
    reach = np.cumsum(counts[::-1])[::-1]
    return max(1, int(np.argmax(reach <= len(flat) // 10)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 28)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, Plan, Reads, RunEncoder, ViewEncoder, make_params
    from bamsignals_amd.synth import synth_reads
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured without one")
    ctx = Context(0)
    # (a) the coverage of two whole references
    ref_len = [2_000_000, 700_017]
    cols = synth_reads(400_000, ref_len, seed=92, paired=True)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                  cigar_off=cols["cigar_off"], cigar=cols["cigar"])
    plan = Plan(ctx, reads, [0, 1], [0, 0], ref_len, [1, 1], make_params(_lib.MODE_COVERAGE))
    buf = torch.empty(plan.cells, dtype=torch.int32, device="cuda:0")
    plan.run_device(buf.data_ptr())
    ctx.sync()
    views, runs = plan.views(), plan.runs()
    measure("coverage of 2 Mbp + 700 kbp", ctx, views, runs, buf.data_ptr(), plan.cells, 2, decile(buf.cpu().numpy()), a.steps, a.warmup)
    for o in (views, runs, plan, reads):
        o.close()
    del buf
    # (b) the synthetic buffer
    n = a.cells
    g = torch.Generator(device="cuda:0").manual_seed(7)
    coarse = torch.randint(0, 40, (n // 32 + n // 512 + 64,), generator=g, device="cuda:0", dtype=torch.int32)
    reps = torch.randint(1, 64, (n // 32 + n // 512 + 64,), generator=g, device="cuda:0")
    buf = torch.repeat_interleave(coarse, reps)[:n].contiguous()
    del coarse, reps
    assert buf.numel() == n
    torch.cuda.synchronize()
    base = np.arange(4, dtype=np.int64) * (n // 4)
    length = np.full(4, n // 4, np.int32)
    views, runs = ViewEncoder(ctx, base, length, 1), RunEncoder(ctx, base, length, 1)
    measure(f"synthetic, {n} cells", ctx, views, runs, buf.data_ptr(), int(length.sum()), 4, 36, a.steps, a.warmup)
    views.close()
    runs.close()
    ctx.close()


if __name__ == "__main__":
    main()
