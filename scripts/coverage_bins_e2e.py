#!/usr/bin/env python3
"""End-to-end seconds of a resident file-level bamCoverage call (the BAM already decoded in HBM), per base and in
bins: one whole-reference range of a seeded synthetic BAM at config 3's read density (0.4 reads a base).  Prints
one JSON line per case: the median of the warm calls and where their time went (bsig_last_call_timing_ex)."""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from bamsignals_amd import GRanges, bamCoverage
    from bamsignals_amd.bamio import write_columns_as_bam
    from bamsignals_amd.synth import synth_reads
    from bamsignals_amd.wrappers import last_call_timing

    L = int(os.environ.get("COVERAGE_E2E_BP", "50000000"))
    n = int(0.4 * L)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cov.bam")
        cols = synth_reads(n, [L], seed=3)
        write_columns_as_bam(path, ["chr1"], cols)
        del cols
        gr = GRanges("chr1", [1], width=[L])
        bamCoverage(path, gr, verbose=False)                # the cold call decodes the BAM into HBM
        for name, kw in (("per base", {}), ("binsize=50", dict(binsize=50)), ("binsize=1000", dict(binsize=1000)),
                         ("binsize=50, ss", dict(binsize=50, ss=True))):
            ts, parts = [], []
            for _ in range(6):
                t0 = time.perf_counter()
                sig = bamCoverage(path, gr, verbose=False, **kw)
                ts.append(time.perf_counter() - t0)
                parts.append(last_call_timing())
            k = int(np.argsort(ts[1:])[len(ts[1:]) // 2]) + 1
            p = parts[k]
            print(json.dumps(dict(case=f"bamCoverage {name}, ONE {L:,}-bp range, {n:,} reads, resident", call_ms=1e3 * ts[k],
                                  result_bytes=int(sum(s.nbytes for s in sig.as_list())), resident=p["bam_was_resident"],
                                  plan_ms=1e3 * p["plan"], kernels_ms=1e3 * p["kernels"], download_ms=1e3 * p["download"])),
                  flush=True)


if __name__ == "__main__":
    main()
