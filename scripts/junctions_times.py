#!/usr/bin/env python3
"""bamJunctions on one GPU: the resident query, and what building the junction table adds to making a spliced set.

The workload is the junction deck's generator (tests/junctions_expected.py) scaled up and vectorised: --genes genes on four
references, 3-8 exons of 30-200 bases, introns of 80-20,000 (log-uniform), --reads reads of 100 transcript bases spread over
the genes, every inner exon skipped with probability 0.15, strand by gene with 10 % flipped, 3 % 0x400, mapq of {0, 3, 30, 60}.

  query   (this process) the set uploaded spliced; Reads.junctions for one range per reference and for the gene ranges,
          without and with a filter: HIP events over --steps after --warmup, median / min / max in ms.  Beside it the numpy
          restatement on this host's CPU (np.unique over the same filtered rows, the rows given): the only comparable figure.
  build   (child processes, one per library and run, alternating) Reads(spliced=True) of the same columns, and the cold
          bamCoverage(splice=True) of a BAM written from the first --bam-reads of them, under this commit's library and
          under --parent-lib (BSIG_LIB_PATH: a parent commit's build without the table): seconds, every run listed, so the
          difference stands beside the parent's own run-to-run spread.

Prints one JSON line per measurement.

  python scripts/junctions_times.py [--reads 20000000] [--genes 20000] [--steps 30] [--warmup 5] [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REF_LEN = 250_000_000
N_REF = 4
SLOT = 48_000
READ_BASES = 100


def gene_model_reads(n_reads, n_genes, seed):
    """(CIGAR columns, gene ranges): the deck's generator on arrays"""
    rng = np.random.default_rng(seed)
    n_exon = rng.integers(3, 9, n_genes)
    exons = rng.integers(30, 201, (n_genes, 8))
    exons[np.arange(8)[None, :] >= n_exon[:, None]] = 0
    introns = np.exp(rng.uniform(np.log(80), np.log(20_000), (n_genes, 8))).astype(np.int64).clip(80, 20_000)
    introns[np.arange(8)[None, :] >= (n_exon - 1)[:, None]] = 0
    # a gene that does not fit its slot gets its introns scaled down (the deck redraws; the shape of the load is the same)
    span = exons.sum(1) + introns.sum(1)
    scale = np.minimum(1.0, (SLOT - 4_000) / span)
    introns = np.where(introns > 0, np.maximum((introns * scale[:, None]).astype(np.int64), 80), 0)
    per_ref = (n_genes + N_REF - 1) // N_REF
    assert per_ref * SLOT <= REF_LEN
    g_rid = (np.arange(n_genes) // per_ref).astype(np.int32)
    first = (np.arange(n_genes) % per_ref) * SLOT + 1_000 + rng.integers(0, 500, n_genes)
    ex_start = first[:, None] + np.concatenate([np.zeros((n_genes, 1), np.int64), np.cumsum(exons[:, :-1] + introns[:, :-1], axis=1)], axis=1)
    g_minus = rng.integers(0, 2, n_genes).astype(bool)
    last = ex_start[np.arange(n_genes), n_exon - 1] + exons[np.arange(n_genes), n_exon - 1] - 1
    genes = dict(rid=g_rid, loc=first.astype(np.int32), len=(last - first + 1).astype(np.int32), strand=np.where(g_minus, -1, 1).astype(np.int32))
    # reads
    gene = np.sort(rng.integers(0, n_genes, n_reads))
    L = exons[gene].astype(np.int32)
    k = np.arange(8)[None, :]
    inner = (k >= 1) & (k < (n_exon[gene] - 1)[:, None])
    L[inner & (rng.random((n_reads, 8)) < 0.15)] = 0
    T1 = np.cumsum(L, axis=1, dtype=np.int32)
    T0 = T1 - L
    t_len = T1[:, -1]
    ln = np.minimum(READ_BASES, t_len)
    at = (rng.random(n_reads) * (t_len - ln + 1)).astype(np.int32)
    ov = np.clip(np.minimum(T1, (at + ln)[:, None]) - np.maximum(T0, at[:, None]), 0, None).astype(np.int32)
    p_start = ex_start[gene] + np.clip(at[:, None] - T0, 0, None)
    p_end = p_start + ov - 1
    has = ov > 0
    pos = np.where(has, p_start, np.iinfo(np.int64).max).min(axis=1)
    order = np.lexsort((pos, g_rid[gene]))
    gene, ov, p_start, p_end, has, pos = gene[order], ov[order], p_start[order], p_end[order], has[order], pos[order]
    # the end of the covered piece before each piece: a running maximum along the exons
    prev_end = np.maximum.accumulate(np.where(has, p_end, -1), axis=1)
    prev_end = np.concatenate([np.full((n_reads, 1), -1, np.int64), prev_end[:, :-1]], axis=1)
    gap = np.where(has & (prev_end >= 0), p_start - prev_end - 1, 0)
    ops = np.zeros((n_reads, 16), dtype=np.uint32)
    ops[:, 0::2] = (gap.astype(np.uint32) << 4) | 3
    ops[:, 1::2] = (ov.astype(np.uint32) << 4) | 0
    valid = np.zeros((n_reads, 16), dtype=bool)
    valid[:, 0::2] = gap > 0
    valid[:, 1::2] = has
    rev = g_minus[gene] != (rng.random(n_reads) < 0.10)
    flag = (np.where(rev, 16, 0) | np.where(rng.random(n_reads) < 0.03, 0x400, 0)).astype(np.uint16)
    rid = g_rid[gene]
    cols = dict(ref_len=np.full(N_REF, REF_LEN, np.int32), ref_off=np.searchsorted(rid, np.arange(N_REF + 1)).astype(np.int64),
                pos=pos.astype(np.int32), flag=flag, mapq=rng.choice(np.asarray([0, 3, 30, 60], np.uint8), n_reads),
                tlen=np.zeros(n_reads, np.int32), cigar_off=np.concatenate([[0], np.cumsum(valid.sum(1))]).astype(np.int64),
                cigar=ops[valid], end=np.where(has, p_end, -1).max(axis=1).astype(np.int32))
    # the junction rows, for the restatement's time: (ref, start, end, flag, mapq, anchor)
    left = np.zeros_like(ov)            # the covered piece before each exon, carried over the exons a read skips
    run = np.zeros(n_reads, dtype=ov.dtype)
    for j in range(8):
        left[:, j] = run
        run = np.where(has[:, j], ov[:, j], run)
    is_gap = gap > 0
    rows = dict(ref=np.broadcast_to(rid[:, None], is_gap.shape)[is_gap].astype(np.int64), start=(prev_end + 1)[is_gap], end=(p_start - 1)[is_gap],
                flag=np.broadcast_to(flag[:, None], is_gap.shape)[is_gap].astype(np.int64),
                mapq=np.broadcast_to(cols["mapq"][:, None], is_gap.shape)[is_gap].astype(np.int64),
                anchor=np.minimum(left, ov)[is_gap].astype(np.int64))
    return cols, genes, rows


def restated(rows, rg, mapqual=0, filteredF=-1, min_anchor=0):
    """np.unique over the filtered rows of every range (one range per reference, or the genes: rows inside by construction)"""
    nf = ~rows["flag"]
    keep = (rows["mapq"] >= mapqual) & ((filteredF & nf & 0xFFFFFFFF) != 0) & (rows["anchor"] >= min_anchor)
    key = (rows["ref"][keep] << 56) | (rows["start"][keep] << 28) | rows["end"][keep]
    u, c = np.unique(key, return_counts=True)
    return len(u), int(c.sum())


def child(a):
    """one run of the build stage under whatever library BSIG_LIB_PATH names"""
    from bamsignals_amd import GRanges, _lib, bamCoverage
    from bamsignals_amd.device import Context, Reads
    cols = dict(np.load(a.child))
    ctx = Context(0)
    times = []
    for _ in range(a.uploads + 1):
        t0 = time.perf_counter()
        r = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                  cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=True)
        ctx.sync()
        times.append(time.perf_counter() - t0)
        hbm, blocks = r.info()["hbm_bytes"], r.info()["n_reads"]
        rows = r.n_junction_rows if hasattr(_lib.load(), "bsig_reads_junctions") else None
        r.close()
    gr = GRanges([f"chr{k + 1}" for k in range(N_REF)], np.ones(N_REF), width=np.full(N_REF, 1_000_000))
    _lib.load().bsig_cache_clear()
    t0 = time.perf_counter()
    bamCoverage(a.bam, gr, verbose=False, splice=True)
    cold = time.perf_counter() - t0
    print(json.dumps(dict(what="build", library=os.path.relpath(_lib.SO_PATH, ROOT), upload_s=[round(t, 4) for t in times[1:]],
                          first_upload_s=round(times[0], 4), cold_coverage_s=round(cold, 4), hbm_bytes=hbm, blocks=blocks,
                          junction_rows=rows)), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--genes", type=int, default=20_000)
    ap.add_argument("--bam-reads", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--uploads", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--bam", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)

    t0 = time.perf_counter()
    cols, genes, rows = gene_model_reads(a.reads, a.genes, a.seed)
    print(json.dumps(dict(what="workload", reads=a.reads, genes=a.genes, junction_rows=len(rows["start"]),
                          generated_s=round(time.perf_counter() - t0, 1))), flush=True)
    with tempfile.TemporaryDirectory() as d:
        # ---- build: child processes, alternating libraries (before this process opens the GPU) -----------------------
        from bamsignals_amd.bamio import write_columns_as_bam
        npz, bam = os.path.join(d, "cols.npz"), os.path.join(d, "genes.bam")
        np.savez(npz, **cols)
        m = min(a.bam_reads, a.reads)
        sub = dict(cols, ref_off=np.minimum(cols["ref_off"], m), pos=cols["pos"][:m], flag=cols["flag"][:m], mapq=cols["mapq"][:m],
                   tlen=cols["tlen"][:m], end=cols["end"][:m], cigar_off=cols["cigar_off"][:m + 1], cigar=cols["cigar"][:cols["cigar_off"][m]])
        write_columns_as_bam(bam, [f"chr{k + 1}" for k in range(N_REF)], sub)
        libs = [""] + ([os.path.abspath(a.parent_lib)] if a.parent_lib else [])
        for _ in range(a.runs):
            for lib in libs:
                env = dict(os.environ)
                env.pop("BSIG_LIB_PATH", None)
                if lib:
                    env["BSIG_LIB_PATH"] = lib
                env["BAMSIGNALS_DECODE"] = "all"        # (the cold call decodes the whole file, whatever the ranges)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", npz, "--bam", bam, "--uploads", str(a.uploads)],
                               env=env, check=True, timeout=600)

    # ---- query -----------------------------------------------------------------------------------------------------------
    import torch

    from bamsignals_amd.device import Context, Reads
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                  cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=True)
    assert reads.n_junction_rows == len(rows["start"])
    whole = dict(rid=np.arange(N_REF, dtype=np.int32), loc=np.zeros(N_REF, np.int32), len=np.full(N_REF, REF_LEN, np.int32),
                 strand=np.zeros(N_REF, np.int32))
    for what, rg in (("one range per reference", whole), (f"{a.genes} gene ranges", genes)):
        for flt in (dict(), dict(mapqual=30, filteredF=0x400, min_anchor=8)):
            for run in range(a.runs):
                ms = []
                for i in range(a.warmup + a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    got = reads.junctions(rg["rid"], rg["loc"], rg["len"], rg["strand"], ss=True, **flt)
                    e1.record(stream)
                    e1.synchronize()
                    if i >= a.warmup:
                        ms.append(e0.elapsed_time(e1))
                t0 = time.perf_counter()
                n_distinct, n_kept = restated(rows, rg, **flt)
                cpu_ms = (time.perf_counter() - t0) * 1e3
                assert len(got[1]) == n_distinct and int(got[3].sum()) == n_kept, (len(got[1]), n_distinct, int(got[3].sum()), n_kept)
                print(json.dumps(dict(what="query", ranges=what, filter=flt, run=run, junctions=n_distinct, rows_kept=n_kept,
                                      gpu_ms=(round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)),
                                      numpy_unique_ms=round(cpu_ms, 1))), flush=True)
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
