#!/usr/bin/env python3
"""bamGeneCounts on one GPU: the resident query, the read table's bytes, and what keeping the table adds to making a
spliced set.

The workload is that of scripts/junctions_times.py (same generator, same seed): --genes genes on four references, 3-8 exons
each, --reads reads of 100 transcript bases.  The annotation is made from the same seed: every gene's exons, and a second
transcript of every gene whose exons are the first one's with both ends moved by up to 10 bases (overlapping exons of one
gene, which the flatten collapses) -- about 11 exons a gene.

  query   (this process) the set uploaded spliced, the model flattened on the host (its seconds are printed); then
          Reads.gene_counts under the three strand modes, without and with a filter: HIP events over --steps after --warmup,
          median / min / max in ms (the first query of a model uploads its tables: it is a warm-up step).  Beside it one
          spliced upload of the same set, timed the same way: the one thing to explain would be a query slower than that.
  build   (child processes, one per library and run, alternating) Reads(spliced=True) of the same columns under this
          commit's library and under --parent-lib (BSIG_LIB_PATH: a parent commit's build without the read table): seconds,
          every run listed, and hbm_bytes, so the difference stands beside the parent's own run-to-run spread.

Prints one JSON line per measurement.

  python scripts/genecounts_times.py [--reads 20000000] [--genes 20000] [--steps 30] [--warmup 5] [--parent-lib PATH]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import junctions_times as jt  # noqa: E402

MODES = ("unstranded", "forward", "reverse")


def annotation(n_genes, seed, genes):
    """The exons of junctions_times.gene_model_reads(.., n_genes, seed): its first draws repeated (checked against the gene
    ranges it returned), then the second transcripts: dict(rid, loc, len, strand), gene"""
    rng = np.random.default_rng(seed)
    n_exon = rng.integers(3, 9, n_genes)
    exons = rng.integers(30, 201, (n_genes, 8))
    exons[np.arange(8)[None, :] >= n_exon[:, None]] = 0
    introns = np.exp(rng.uniform(np.log(80), np.log(20_000), (n_genes, 8))).astype(np.int64).clip(80, 20_000)
    introns[np.arange(8)[None, :] >= (n_exon - 1)[:, None]] = 0
    span = exons.sum(1) + introns.sum(1)
    scale = np.minimum(1.0, (jt.SLOT - 4_000) / span)
    introns = np.where(introns > 0, np.maximum((introns * scale[:, None]).astype(np.int64), 80), 0)
    per_ref = (n_genes + jt.N_REF - 1) // jt.N_REF
    first = (np.arange(n_genes) % per_ref) * jt.SLOT + 1_000 + rng.integers(0, 500, n_genes)
    ex_start = first[:, None] + np.concatenate([np.zeros((n_genes, 1), np.int64), np.cumsum(exons[:, :-1] + introns[:, :-1], axis=1)], axis=1)
    has = exons > 0
    g = np.broadcast_to(np.arange(n_genes)[:, None], has.shape)[has]
    loc, ln = ex_start[has], exons[has].astype(np.int64)
    last = np.zeros(n_genes, np.int64)
    np.maximum.at(last, g, loc + ln - 1)
    assert np.array_equal(first, genes["loc"]) and np.array_equal(last - first + 1, genes["len"]), "the replay is the workload's own exons"
    other = np.random.default_rng(seed + 1)
    d0, d1 = other.integers(-10, 11, len(loc)), other.integers(-10, 11, len(loc))
    loc2 = loc + d0
    ln2 = np.maximum(ln - d0 + d1, 1)
    gene = np.concatenate([g, g]).astype(np.int32)
    feats = dict(rid=genes["rid"][gene], loc=np.concatenate([loc, loc2]).astype(np.int32), len=np.concatenate([ln, ln2]).astype(np.int32),
                 strand=genes["strand"][gene])
    return feats, gene


def child(a):
    """one run of the build stage under whatever library BSIG_LIB_PATH names"""
    from bamsignals_amd import _lib
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
        source = r.n_source_reads if hasattr(_lib.load(), "bsig_reads_gene_counts") else None
        r.close()
    print(json.dumps(dict(what="build", library=os.path.relpath(_lib.SO_PATH, ROOT), upload_s=[round(t, 4) for t in times[1:]],
                          first_upload_s=round(times[0], 4), hbm_bytes=hbm, blocks=blocks, source_reads=source)), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--genes", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--uploads", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)

    t0 = time.perf_counter()
    cols, genes, _ = jt.gene_model_reads(a.reads, a.genes, a.seed)
    feats, gene = annotation(a.genes, a.seed, genes)
    print(json.dumps(dict(what="workload", reads=a.reads, genes=a.genes, exons=len(gene), generated_s=round(time.perf_counter() - t0, 1))),
          flush=True)
    with tempfile.TemporaryDirectory() as d:
        # ---- build: child processes, alternating libraries (before this process opens the GPU) -----------------------
        npz = os.path.join(d, "cols.npz")
        np.savez(npz, **cols)
        libs = [""] + ([os.path.abspath(a.parent_lib)] if a.parent_lib else [])
        for _ in range(a.runs):
            for lib in libs:
                env = dict(os.environ)
                env.pop("BSIG_LIB_PATH", None)
                if lib:
                    env["BSIG_LIB_PATH"] = lib
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", npz, "--uploads", str(a.uploads)], env=env, check=True,
                               timeout=600)

    # ---- query -----------------------------------------------------------------------------------------------------------
    import torch

    from bamsignals_amd import GeneModel
    from bamsignals_amd.device import Context, Reads
    t0 = time.perf_counter()
    model = GeneModel.from_arrays(feats["rid"], feats["loc"], feats["len"], feats["strand"], gene, a.genes, jt.N_REF)
    print(json.dumps(dict(what="flatten", exons=len(gene), host_s=round(time.perf_counter() - t0, 3),
                          segments={t: model.n_segments(t) for t in ("unstranded", "plus", "minus")})), flush=True)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = Context(0, stream=stream.cuda_stream)

    def timed(fn):
        ms, got = [], None
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            got = fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return got, (round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3))

    def up():
        r = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                  cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=True)
        r.close()

    _, ms = timed(up)
    print(json.dumps(dict(what="upload", gpu_ms=ms)), flush=True)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                  cigar_off=cols["cigar_off"], cigar=cols["cigar"], spliced=True)
    n_blocks = reads.info()["n_reads"]
    print(json.dumps(dict(what="table", source_reads=reads.n_source_reads, blocks=n_blocks,
                          bytes=8 * (reads.n_source_reads + 1) + 8 * n_blocks + 8 * (jt.N_REF + 1), hbm_bytes=reads.info()["hbm_bytes"])), flush=True)
    for mode in MODES:
        for flt in (dict(), dict(mapqual=30, filteredF=0x400)):
            for run in range(a.runs):
                (counts, summary), ms = timed(lambda: reads.gene_counts(model, strand=mode, **flt))
                assert summary.sum() == a.reads and counts.sum() == summary[0]
                if mode == "unstranded" and not flt:
                    # every read of this workload lies on exons of its own gene, and every gene has a slot of its own
                    assert summary.tolist() == [a.reads, 0, 0, 0, 0], summary
                print(json.dumps(dict(what="query", strand=mode, filter=flt, run=run, summary=summary.tolist(),
                                      genes_with_reads=int(np.count_nonzero(counts)), gpu_ms=ms)), flush=True)
    reads.close()
    ctx.close()


if __name__ == "__main__":
    main()
