#!/usr/bin/env python3
"""Strand cross-correlation (bsig_plan_run_xcorr, bamCrossCorr) timed on one GPU, in one process.

(a) The resident xcorr step over whole references of reads at the bench's north-star density (0.2 reads a base), at
    several lags, alternated with the per-range strand-split step (bsig_plan_run, ss) over the same bases: HIP events
    over --steps after --warmup.  With each: the step's multiply-adds nnz(S) * (maxlag + 1), counted from the
    per-range result (the non-zero sense cells of every range), and the plan's algorithmic bytes.
(b) The file-level bamCrossCorr(maxlag=500) over one reference of a BAM of those reads against the route the library
    offered before: bamProfile(ss=True) over that reference and the maxlag + 1 int64 dot products in numpy, wall clock,
    alternated, --calls each, the results compared.

Prints one JSON line per measurement.

  python scripts/xcorr_times.py [--refs 1] [--ref-len 250000000] [--steps 20] [--warmup 3] [--calls 3] [--lags 100,500,2047]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_cross(sig, maxlag):
    """the dot products of the earlier route: S[:w - d] . A[d:] in int64, per lag"""
    s, a = np.asarray(sig[0], np.int64), np.asarray(sig[1], np.int64)
    w = len(s)
    return np.asarray([np.dot(s[:w - d], a[d:]) for d in range(maxlag + 1)], np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=1, help="references of --ref-len bases (the bench's genome has 10)")
    ap.add_argument("--ref-len", type=int, default=250_000_000)
    ap.add_argument("--density", type=float, default=0.2, help="reads a base (the north star: 5e8 reads on 2.5 Gbp)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--lags", default="100,500,2047")
    ap.add_argument("--skip-file", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import GRanges, _lib, bamCrossCorr, bamProfile, write_columns_as_bam
    from bamsignals_amd.device import Context, Plan, Reads, XcorrPlan, make_params
    from bamsignals_amd.synth import add_cigar
    from bamsignals_amd.wrappers import last_call_timing

    ref_len = [a.ref_len] * a.refs
    n_reads = int(a.density * a.ref_len * a.refs)
    cols = bench.make_reads(n_reads, ref_len, a.seed, False)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    rg = dict(rid=np.arange(a.refs, dtype=np.int32), loc=np.zeros(a.refs, np.int32), len=np.asarray(ref_len, np.int32),
              strand=np.ones(a.refs, np.int32))
    prm = make_params(_lib.MODE_PROFILE, ss=True)
    per = Plan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], prm)
    out = torch.empty(per.cells, dtype=torch.int32, device="cuda:0")
    per.run_device(out.data_ptr())
    stream.synchronize()
    nnz = int(torch.count_nonzero(out[0::2]).item())          # non-zero sense cells
    base = dict(refs=a.refs, ref_len=a.ref_len, reads=n_reads, nnz_sense=nnz)
    for maxlag in [int(x) for x in a.lags.split(",")]:
        xp = XcorrPlan(ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"], make_params(_lib.MODE_PROFILE), maxlag)
        res = torch.empty(xp.cells, dtype=torch.int64, device="cuda:0")
        times = {"xcorr": [], "per_range_ss": []}
        for k in range(a.warmup + a.steps):
            for key, fn in (("xcorr", lambda: xp.run_device(res.data_ptr())), ("per_range_ss", lambda: per.run_device(out.data_ptr()))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if k >= a.warmup:
                    times[key].append(e0.elapsed_time(e1))
        st_x, st_p = xp.stats(), per.stats()
        ms_x, ms_p = float(np.median(times["xcorr"])), float(np.median(times["per_range_ss"]))
        macs = nnz * (maxlag + 1)
        got = res.cpu().numpy()
        print(json.dumps(dict(base, what="resident step", maxlag=maxlag, xcorr_ms=round(ms_x, 3), xcorr_min_ms=round(min(times["xcorr"]), 3),
                              xcorr_max_ms=round(max(times["xcorr"]), 3), per_range_ss_ms=round(ms_p, 3),
                              multiply_adds=macs, gmacs_per_s=round(macs / (ms_x * 1e-3) / 1e9, 1),
                              B_xcorr_MB=round(st_x["algorithmic_bytes"] / 1e6, 1), B_per_range_MB=round(st_p["algorithmic_bytes"] / 1e6, 1),
                              tiles=st_x["n_items"], heavy_tiles=st_x["heavy_tiles"], argmax=int(np.argmax(got[:maxlag + 1])),
                              sums=[int(v) for v in got[maxlag + 1:]])), flush=True)
        xp.close()
        del res
    per.close()
    del out
    reads.close()
    ctx.close()
    if a.skip_file:
        return

    # (b) one reference through a BAM file
    one = int(cols["ref_off"][1])
    sub = {k: np.ascontiguousarray(cols[k][:one]) for k in ("pos", "flag", "mapq", "tlen", "end", "cigar_menu") if k in cols}
    sub["ref_len"], sub["ref_off"] = np.asarray(ref_len[:1], np.int32), np.asarray([0, one], np.int64)
    if "cigar_menu" in sub:
        add_cigar(sub)
    else:
        sub["cigar_off"] = np.arange(one + 1, dtype=np.int64)
        sub["cigar"] = ((sub["end"].astype(np.int64) - sub["pos"] + 1) << 4).astype(np.uint32)
    del cols
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "one_ref.bam")
        write_columns_as_bam(bam, ["chr1"], sub)
        gr = GRanges(["chr1"], [1], width=[a.ref_len], strand=["+"])
        bamCrossCorr(bam, gr, maxlag=500, verbose=False)       # (the decode: both routes then find the BAM resident)
        new, old, parts = [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            cc = bamCrossCorr(bam, gr, maxlag=500, verbose=False)
            new.append(time.perf_counter() - t0)
            tn = last_call_timing()
            t0 = time.perf_counter()
            sig = bamProfile(bam, gr, ss=True, verbose=False)
            t1 = time.perf_counter()
            want = host_cross(sig[0], 500)
            t2 = time.perf_counter()
            old.append(t2 - t0)
            parts.append((round(t1 - t0, 3), round(t2 - t1, 3)))
            assert np.array_equal(cc.cross, want)
            del sig
        print(json.dumps(dict(what="file level, one reference, maxlag 500", ref_len=a.ref_len, reads=one,
                              bamCrossCorr_s=[round(t, 4) for t in new], bamProfile_plus_numpy_s=[round(t, 3) for t in old],
                              bamProfile_s_and_dots_s=parts, median_new_s=round(float(np.median(new)), 4),
                              median_old_s=round(float(np.median(old)), 3), equal=True, fragment_length=cc.fragment_length(),
                              last_call_timing={k: (round(v, 5) if isinstance(v, float) else v) for k, v in tn.items()})), flush=True)
        _lib.load().bsig_cache_clear()


if __name__ == "__main__":
    main()
