#!/usr/bin/env python3
"""bamOverlaps (an overlap plan: type "any", minoverlap 1) timed against bamCount on one GPU, in one process.

Resident synthetic single-end reads on one reference at BASELINE config 3's density (1e8 reads on chr1's 248,956,422 bp);
two sets of ranges: config 3's tiling in 2-kb tiles, which is what scripts/profile_case.py times bamCount on, and --peaks
200-bp ranges.  For each set the resident step of three plans over the same ranges, alternated inside one loop: a COUNT
plan (the yardstick: the same windows, the same bytes per visit), an overlap plan, and an overlap plan made under
BAMSIGNALS_OVERLAP_QUAD=0, whose packed reads take the per-read 64-bit body instead of OverlapOne::quad.  HIP events over
--steps after --warmup; median, min and max in ms, and the ratios of the medians.  --paired: paired reads and, beside
these, the three plans with requiredF 66 and tlen_filter (0, 1000), the overlap ones with "extend" (their windows reach
out by 1,000 bases: more visits than the count's).

BSIG_LIB_PATH selects another build of the library (a parent commit's: only its COUNT plan is timed then, which says
whether this commit changed bamCount's time).  The launch log names the kernel forms each plan ran.

Prints one JSON line per measurement.

  python scripts/overlaps_times.py [--ref-len 248956422] [--density 0.4] [--peaks 500000] [--steps 30] [--warmup 5] [--paired]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=248_956_422)
    ap.add_argument("--density", type=float, default=0.4, help="reads a base (config 3: 1e8 reads on chr1)")
    ap.add_argument("--peaks", type=int, default=500_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--paired", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()

    import torch

    import bench
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, Plan, Reads, make_params
    from bamsignals_amd.synth import synth_ranges, tile_ranges

    lib = _lib.load()
    has_overlap = hasattr(lib, "bsig_overlap_core")              # (a parent commit's library: the yardstick alone)
    log = lib.bsig_debug_launch_log
    log.argtypes, log.restype = [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    buf = ctypes.create_string_buffer(65537)

    ref_len = [a.ref_len]
    n_reads = int(a.density * a.ref_len) & ~1
    cols = bench.make_reads(n_reads, ref_len, a.seed, a.paired)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], end=cols["end"])
    sets = {"tiling_2kb": tile_ranges(ref_len, 2000), "peaks_200bp": synth_ranges(a.peaks, 200, ref_len, seed=a.seed + 2)}
    base = dict(library=os.path.basename(_lib.SO_PATH), ref_len=a.ref_len, reads=n_reads, paired=bool(a.paired))

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

    rules = [("reads", dict(), dict())]
    if a.paired:
        pe = dict(requiredF=66, tlen_filter=(0, 1000))
        rules.append(("extend", pe, dict(pe, tspan=True)))
    for name, rg in sets.items():
        for rule, count_kw, overlap_kw in rules:
            args = (ctx, reads, rg["rid"], rg["loc"], rg["len"], rg["strand"])
            plans = {"count": Plan(*args, make_params(_lib.MODE_COUNT, binsize=-1, **count_kw))}
            if has_overlap:
                plans["overlap"] = Plan(*args, make_params(_lib.MODE_OVERLAP_ANY, binsize=1, **overlap_kw))
                os.environ["BAMSIGNALS_OVERLAP_QUAD"] = "0"
                plans["overlap_no_quad"] = Plan(*args, make_params(_lib.MODE_OVERLAP_ANY, binsize=1, **overlap_kw))
                os.environ.pop("BAMSIGNALS_OVERLAP_QUAD")
            outs = {k: torch.empty(max(p.cells, 4), dtype=torch.int32, device="cuda:0") for k, p in plans.items()}
            fns = {k: (lambda k=k: plans[k].run_device(outs[k].data_ptr())) for k in plans}
            t = timed(fns)
            forms = {}
            log(None, 1)
            for k, fn in fns.items():
                fn()
                stream.synchronize()
                log(buf, len(buf))
                forms[k] = buf.value.decode().splitlines()
            log(None, 0)
            st = {k: p.stats() for k, p in plans.items()}
            line = dict(base, what="resident step", ranges=name, n_ranges=len(rg["rid"]), rule=rule, forms=forms,
                        tiles=st["count"]["n_items"], **{k + "_ms": v for k, v in t.items()},
                        **{k + "_visits": s["visits"] for k, s in st.items()},
                        **{k + "_MB": round(s["algorithmic_bytes"] / 1e6, 1) for k, s in st.items()},
                        count_total=int(outs["count"].to(torch.int64).sum().item()))
            if has_overlap:
                same = bool(torch.equal(outs["overlap"], outs["overlap_no_quad"]))
                line.update(overlap_over_count=round(t["overlap"][0] / t["count"][0], 3),
                            no_quad_over_count=round(t["overlap_no_quad"][0] / t["count"][0], 3),
                            overlap_total=int(outs["overlap"].to(torch.int64).sum().item()), quad_and_no_quad_agree=same)
            print(json.dumps(line), flush=True)
            for p in plans.values():
                p.close()
            del outs
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
