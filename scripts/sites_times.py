"""Times of bamSites on one GPU against what it replaces -> profiles/sites_times.md (none of them gates anything).

The workload is that of scripts/nucleotides_times.py -- ``--reads`` reads of 100 bases (default 20,000,000) on three references of
688 Mb against ``--ranges`` ranges of ``--width`` bases (default 50,000 x 2,000) -- but the set is built from columns
(``Reads(..., bases=True)``: no file is written) and the reads SAY something: every read is ``100M`` and copies a seeded random
reference, with 0.5 % substitutions and a het SNP every 1,000 bases (half of the reads that cover it show the other allele).
Measured in one job: ``Reads.sites`` into host memory; ``Reads.nucleotides`` into host memory followed by the same filter in
numpy (the baseline: what had to be done before); and both on the device alone (the site query's count + scan and fill stages
as the result handle states them, the dense query with HIP events into device memory).  The two answers are compared.

    python scripts/sites_times.py [--reads N] [--ranges K] [--width W] [--steps S] [--out profiles/sites_times.md]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bamsignals_amd import _lib  # noqa: E402
from bamsignals_amd.device import Context, Reads  # noqa: E402
from bamsignals_amd.synth import synth_ranges  # noqa: E402

READ_LEN = 100
COMP = np.array([3, 2, 1, 0, 4, 5], dtype=np.uint8)


def spread(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:.3f} ({xs[0]:.3f} - {xs[-1]:.3f})"


def make_reads(n_reads, ref_len, seed):
    """(columns for Reads(..., bases=True), the genome's channel codes laid reference after reference)"""
    rng = np.random.default_rng(seed)
    ref_len = np.asarray(ref_len, dtype=np.int64)
    gstart = np.concatenate([[0], np.cumsum(ref_len)])
    genome = rng.integers(0, 4, int(gstart[-1]), dtype=np.uint8)
    g = np.sort(rng.integers(0, int(gstart[-1]), n_reads, dtype=np.int64))
    rid = np.searchsorted(gstart, g, side="right") - 1
    pos = np.minimum(g - gstart[rid], ref_len[rid] - READ_LEN)          # (every read inside its reference; the order survives)
    g = gstart[rid] + pos
    codes = np.empty(n_reads * READ_LEN, dtype=np.uint8)
    step = 1_000_000
    for a in range(0, n_reads, step):
        b = min(a + step, n_reads)
        codes[a * READ_LEN:b * READ_LEN] = genome[(g[a:b, None] + np.arange(READ_LEN)[None, :]).reshape(-1)]
    # 0.5 % substitutions: another channel
    at = rng.integers(0, len(codes), int(0.005 * len(codes)))
    codes[at] = (codes[at] + rng.integers(1, 4, len(at)).astype(np.uint8)) & 3
    # a het SNP where the genome's coordinate is 500 modulo 1,000: half of the reads across it show the next channel
    j = (500 - g) % 1000
    k = np.flatnonzero((j < READ_LEN) & (rng.random(n_reads) < 0.5))
    codes[k * READ_LEN + j[k]] = (genome[g[k] + j[k]] + 1) & 3
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)[codes]
    del codes
    seq = nib[0::2] << 4 | nib[1::2]
    del nib
    cols = dict(ref_len=ref_len.astype(np.int32), ref_off=np.searchsorted(rid, np.arange(len(ref_len) + 1)).astype(np.int64),
                pos=pos.astype(np.int32), flag=np.where(rng.random(n_reads) < 0.5, 16, 0).astype(np.uint16),
                mapq=np.full(n_reads, 40, dtype=np.uint8), tlen=np.zeros(n_reads, dtype=np.int32),
                cigar_off=np.arange(n_reads + 1, dtype=np.int64), cigar=np.full(n_reads, READ_LEN << 4, dtype=np.uint32),
                seq_off=np.arange(n_reads + 1, dtype=np.int64) * READ_LEN, seq=seq, qual=np.full(n_reads * READ_LEN, 30, dtype=np.uint8))
    return cols, genome, gstart


def range_ref(rg, genome, gstart):
    """the reference codes of equal-width ranges as they read: (n, width) uint8"""
    w = int(rg["len"][0])
    ref = genome[(gstart[rg["rid"]] + rg["loc"])[:, None] + np.arange(w)[None, :]]
    minus = rg["strand"] < 0
    ref[minus] = COMP[ref[minus][:, ::-1]]
    return np.ascontiguousarray(ref)


def numpy_filter(out, n, w, ss, ref, min_depth, min_alt, num, den, alt_mask, block=2_000):
    """the sites of dense cells (n ranges of one width, the library's layout), as the ABI defines them: (seg_off, pos, alleles,
    counts), in blocks of ranges"""
    planes = 2 if ss else 1
    cells = out[:n * planes * 6 * w].reshape(n, planes, 6, w)
    in_mask = ((alt_mask >> np.arange(6)) & 1).astype(bool)
    per, pos, alleles, counts = np.zeros(n, dtype=np.int64), [], [], []
    for a in range(0, n, block):
        blk = cells[a:a + block]
        c = blk.sum(axis=1, dtype=np.int64) if ss else blk[:, 0].astype(np.int64)           # (m, 6, w)
        depth = c.sum(axis=1)
        b = ref[a:a + block].astype(np.int64) if ref is not None else np.argmax(c, axis=1)
        allowed = in_mask[None, :, None] & (np.arange(6)[None, :, None] != b[:, None, :])
        masked = np.where(allowed, c, -1)
        alt = np.argmax(masked, axis=1)
        ca = np.take_along_axis(masked, alt[:, None, :], axis=1)[:, 0, :]
        site = (depth >= min_depth) & (ca >= min_alt) & (ca * den >= num * depth)
        if ref is not None:
            site &= b != 4
        i, p = np.nonzero(site)
        per[a:a + block] = np.bincount(i, minlength=len(blk))
        pos.append(p.astype(np.int32))
        alleles.append((b[i, p] | alt[i, p] << 8).astype(np.int32))
        counts.append(blk[i, :, :, p])
    seg_off = np.concatenate([[0], np.cumsum(per)])
    counts = np.concatenate(counts)
    return seg_off, np.concatenate(pos), np.concatenate(alleles), counts if ss else counts[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--ranges", type=int, default=50_000)
    ap.add_argument("--width", type=int, default=2_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--min-depth", type=int, default=2)
    ap.add_argument("--min-alt", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "sites_times.md"))
    a = ap.parse_args()
    ref_len = [248_000_000, 242_000_000, 198_000_000]
    t0 = time.perf_counter()
    cols, genome, gstart = make_reads(a.reads, ref_len, seed=3)
    rg = synth_ranges(a.ranges, a.width, cols["ref_len"], seed=4)
    ref = range_ref(rg, genome, gstart)
    lib = _lib.load()
    lines = [f"# bamSites: times ({a.reads:,} reads of {READ_LEN} bases, {a.ranges:,} ranges of {a.width:,})", "",
             f"- the reads: every one {READ_LEN}M, copies of a seeded reference with 0.5 % substitutions and a het SNP every 1,000 bases; made in "
             f"{time.perf_counter() - t0:.1f} s",
             f"- the rule: minDepth {a.min_depth}, minAlt {a.min_alt}, minFraction 1/5, deletions allowed (mask 0x2F)"]
    ctx = Context(0)
    t0 = time.perf_counter()
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"], cigar_off=cols["cigar_off"],
                  cigar=cols["cigar"], bases=True, seq_off=cols["seq_off"], seq=cols["seq"], qual=cols["qual"])
    ctx.sync()
    lines.append(f"- the set from columns: {time.perf_counter() - t0:.2f} s; the base table states {reads.base_table_bytes / 1e6:,.1f} MB")
    del cols
    n, w = len(rg["rid"]), a.width
    ptr = [C.c_void_p(rg[k].ctypes.data) for k in ("rid", "loc", "len", "strand")]
    rule = dict(min_depth=a.min_depth, min_alt=a.min_alt, frac=(1, 5), alt_mask=0x2F)
    for ss in (False, True):
        for use_ref in (True, False):
            what = f"ss={ss}, {'with ref' if use_ref else 'major mode'}"
            flat = ref.reshape(-1) if use_ref else None
            # ---- sites into host memory; the stages on the device alone --------------------------------------------------------
            ms_host, ms_count, ms_fill, ms_down = [], [], [], []
            for step in range(a.steps + 2):
                t3 = []
                t0 = time.perf_counter()
                got = reads.sites(rg["rid"], rg["loc"], rg["len"], rg["strand"], ref=flat, ss=ss, timing=t3, **rule)
                if step >= 2:
                    ms_host.append(1e3 * (time.perf_counter() - t0))
                    ms_count.append(1e3 * t3[0]); ms_fill.append(1e3 * t3[1]); ms_down.append(1e3 * t3[2])
            n_sites = len(got[1])
            back = got[0].nbytes + sum(x.nbytes for x in got[1:])
            # ---- the baseline: the dense table into host memory, then the same filter in numpy ------------------------------------
            cells = int(lib.bsig_nucleotides_cells(n, rg["len"].ctypes.data, int(ss), None))
            out = np.zeros(cells, dtype=np.int32)
            ms_dense, ms_filter = [], []
            for step in range(3):
                t0 = time.perf_counter()
                _lib.check(lib.bsig_reads_nucleotides_host(reads._h, n, *ptr, 0, 0, -1, 0, int(ss), C.c_void_p(out.ctypes.data)))
                t1 = time.perf_counter()
                if step == 0:           # (once: it takes its seconds)
                    want = numpy_filter(out, n, w, ss, ref if use_ref else None, a.min_depth, a.min_alt, 1, 5, 0x2F)
                    ms_filter.append(1e3 * (time.perf_counter() - t1))
                ms_dense.append(1e3 * (t1 - t0))
            same = all(np.array_equal(x, y) for x, y in zip(got, want))
            del out
            # ---- the dense query on the device alone -------------------------------------------------------------------------
            dev = torch.empty(cells, dtype=torch.int32, device="cuda:0")
            ms_dev = []
            for step in range(a.steps + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                _lib.check(lib.bsig_reads_nucleotides(reads._h, n, *ptr, 0, 0, -1, 0, int(ss), C.c_void_p(dev.data_ptr())))
                e1.record()
                torch.cuda.synchronize()
                if step >= 2:
                    ms_dev.append(e0.elapsed_time(e1))
            del dev
            med = lambda xs: sorted(xs)[len(xs) // 2]          # noqa: E731
            base = med(ms_dense) + med(ms_filter)
            lines += [f"- {what}: {n_sites:,} sites of {n * w:,} bases ({back / 1e6:,.1f} MB come back); the filter over the dense table gives "
                      f"{'the same arrays' if same else 'OTHER ARRAYS'}",
                      f"  - sites into host memory: {spread(ms_host)} ms, of which on the device count + scan {spread(ms_count)} ms, fill {spread(ms_fill)} ms; "
                      f"download {spread(ms_down)} ms; the rest is the upload of the ranges{' and of the reference bytes' if use_ref else ''} and the host's checks",
                      f"  - baseline: the dense table into host memory {spread(ms_dense)} ms ({cells * 4 / 1e6:,.0f} MB down), the filter in numpy "
                      f"{spread(ms_filter)} ms: {base:,.0f} ms in all = {base / med(ms_host):,.1f} x sites into host memory "
                      f"({med(ms_dense) / med(ms_host):,.1f} x for the download alone)",
                      f"  - on the device alone: sites {med(ms_count) + med(ms_fill):.3f} ms (two walks, no drain), the dense query {spread(ms_dev)} ms "
                      f"(one walk and the drain): {(med(ms_count) + med(ms_fill)) / med(ms_dev):.2f} x"]
            print("\n".join(lines[-4:]), flush=True)
    reads.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
