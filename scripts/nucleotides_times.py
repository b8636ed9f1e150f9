"""Times of bamNucleotides' stages on one GPU -> profiles/nucleotides_times.md (none of them gates anything).

The workload: a real-shaped BAM (``--reads`` records of 100 bases with qualities, default 20,000,000) against ``--ranges``
ranges of ``--width`` bases (default 50,000 x 2,000).  Measured: the decode + table cold (Reads.from_bam(bases=True): host
decode of the bases, upload, layout, table) against the plain decode of the same file; the resident query with HIP events
(Reads.nucleotides into host memory, and the kernel alone into device memory) with and without minBaseQuality and ss;
hbm_bytes with and without the table; and the bytes the query must move -- the table bytes of the reads the ranges touch
plus 24 x bases written -- so that the distance to HBM speed is readable.

    python scripts/nucleotides_times.py [--reads N] [--ranges K] [--width W] [--steps S] [--out profiles/nucleotides_times.md]
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bamsignals_amd import BamFile, _lib, write_columns_as_bam  # noqa: E402
from bamsignals_amd.device import Context, Reads  # noqa: E402
from bamsignals_amd.synth import synth_ranges, synth_reads  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:.3f} ({xs[0]:.3f} - {xs[-1]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--ranges", type=int, default=50_000)
    ap.add_argument("--width", type=int, default=2_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "nucleotides_times.md"))
    a = ap.parse_args()
    ref_len = [248_000_000, 242_000_000, 198_000_000]
    cols = synth_reads(a.reads, ref_len, seed=3)
    rg = synth_ranges(a.ranges, a.width, cols["ref_len"], seed=4)
    lib = _lib.load()
    lines = [f"# bamNucleotides: stage times ({a.reads:,} reads of 100 bases, {a.ranges:,} ranges of {a.width:,})", ""]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "real.bam")
        t0 = time.perf_counter()
        write_columns_as_bam(path, ["chr1", "chr2", "chr3"], cols, l_seq=100, seed=3)
        lines.append(f"- the file: {os.path.getsize(path) / 1e6:,.1f} MB, written in {time.perf_counter() - t0:.1f} s")
        ctx = Context(0)
        bam = BamFile(path)
        cold = {}
        for name, kw in (("plain", dict()), ("bases", dict(bases=True)), ("plain again", dict()), ("bases again", dict(bases=True))):
            t0 = time.perf_counter()
            r = Reads.from_bam(ctx, bam, **kw)
            ctx.sync()
            cold[name] = (time.perf_counter() - t0, r.info()["hbm_bytes"], r.base_table_bytes)
            if name != "bases again":
                r.close()
        for name, (s, hbm, table) in cold.items():
            lines.append(f"- decode + layout cold, {name}: {s:.3f} s; hbm_bytes {hbm / 1e6:,.1f} MB, of which the base table states {table / 1e6:,.1f} MB")
        reads = r
        n = len(rg["rid"])
        # the bytes the query must move: the table rows, operations, nibbles and qualities of the reads that touch a range, once
        # per range, plus the cells written
        end = cols["end"].astype(np.int64)
        rid_of = np.repeat(np.arange(len(ref_len)), np.diff(cols["ref_off"]))
        touched = ops = 0
        n_ops = np.diff(cols["cigar_off"])
        for ref in range(len(ref_len)):
            sel = np.flatnonzero(rid_of == ref)
            mine = rg["rid"] == ref
            lo, hi = rg["loc"][mine].astype(np.int64), rg["loc"][mine].astype(np.int64) + rg["len"][mine]
            first = np.searchsorted(np.maximum.accumulate(end[sel]), lo, "left")
            last = np.searchsorted(cols["pos"][sel], hi, "left")
            touched += int(np.maximum(last - first, 0).sum())
            cum = np.concatenate([[0], np.cumsum(n_ops[sel])])
            ops += int((cum[np.maximum(last, first)] - cum[first]).sum())
        for ss in (False, True):
            cells = int(lib.bsig_nucleotides_cells(n, rg["len"].ctypes.data, int(ss), None))
            must = touched * (28 + 150) + 4 * ops + 4 * cells
            out = torch.empty(cells, dtype=torch.int32, device="cuda:0")
            for q in (0, 20):
                ms_dev, ms_host = [], []
                for step in range(a.steps + 3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    _lib.check(lib.bsig_reads_nucleotides(reads._h, n, *(C.c_void_p(rg[k].ctypes.data) for k in ("rid", "loc", "len", "strand")),
                                                          0, 0, -1, q, int(ss), C.c_void_p(out.data_ptr())))
                    e1.record()
                    torch.cuda.synchronize()
                    if step >= 3:
                        ms_dev.append(e0.elapsed_time(e1))
                for step in range(3):
                    t0 = time.perf_counter()
                    got = reads.nucleotides(rg["rid"], rg["loc"], rg["len"], rg["strand"], min_base_qual=q, ss=ss)
                    ms_host.append(1e3 * (time.perf_counter() - t0))
                med = sorted(ms_dev)[len(ms_dev) // 2]
                lines.append(f"- resident query, ss={ss}, minBaseQuality={q}: {spread(ms_dev)} ms into device memory (ranges up, one launch); "
                             f"{spread(ms_host)} ms into host memory ({cells * 4 / 1e6:,.0f} MB down); must move {must / 1e6:,.0f} MB "
                             f"({touched:,} (range, read) pairs, {cells:,} cells) = {must / med / 1e6:,.1f} GB/s; "
                             f"counts in all: {sum(int(x.sum()) for x in got):,}")
        reads.close()
        bam.close()
        ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
