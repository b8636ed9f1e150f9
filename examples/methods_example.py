#!/usr/bin/env python3
"""The reference's usage example (its inst/examples/methods_example.R) with the Python host:
counts, profiles and coverage of the fixture BAM over the fixture genes.  Needs an MI355X."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bamsignals_amd import GRanges, bamCount, bamCoverage, bamCrossCorr, bamFragSizes, bamProfile  # noqa: E402

bampath = os.path.join(ROOT, "tests", "golden", "randomBam.bam")
reg = json.load(open(os.path.join(ROOT, "tests", "golden", "regions.json")))
genes = GRanges(reg["chrom"][:20], reg["start"][:20], width=reg["width"][:20], strand=reg["strand"][:20])

# reads whose 5' end falls in each gene; strand-specific: row 0 sense, row 1 antisense
print(bamCount(bampath, genes, verbose=False))
print(bamCount(bampath, genes, ss=True, verbose=False))

# promoters: 100 bp around each gene's start, on the gene's strand
proms = GRanges(genes.seqnames, [max(1, s - 50) for s in genes.start], width=100, strand=genes.strand)
prof = bamProfile(bampath, proms, binsize=1, verbose=False)
print(prof)                               # CountSignals object with 20 signals
print(prof.alignSignals().shape)          # (100, 20): all promoters have the same width
binned = bamProfile(bampath, proms, binsize=20, ss=True, verbose=False)
print(binned[0])                          # 2 x 5 matrix

# paired-end: count fragments at their midpoint, fragments of 50-300 bp only
print(bamCount(bampath, genes, paired_end="midpoint", tlenFilter=(50, 300), verbose=False))

# per-base coverage, fragments extended to the whole template
cov = bamCoverage(bampath, genes, paired_end="extend", verbose=False)
print(cov[0][:20])

# the data's own value for `shift`: the lag at which forward and reverse 5' ends line up best over the genes
cc = bamCrossCorr(bampath, genes, maxlag=300, verbose=False)
print(cc.fragment_length(), cc.fragment_length() // 2)
print(bamCount(bampath, genes, shift=cc.fragment_length() // 2, verbose=False))

# the data's own value for `tlenFilter`: the fragment lengths of the proper pairs over the genes
fs = bamFragSizes(bampath, genes, verbose=False)
print(fs.n, fs.mode(), fs.median(), fs.tlen_filter(0.99))
print(bamCount(bampath, genes, paired_end="midpoint", tlenFilter=fs.tlen_filter(0.99), verbose=False))

# the coverage of the genes as runs (an RleList's form) and as a bedGraph: the per-base cells never leave the GPU
runs = bamCoverage(bampath, genes, runs=True, verbose=False)
print(runs, runs[0][0][:5], runs[0][1][:5])
print(runs.to_bedgraph(os.path.join(os.environ.get("TMPDIR", "/tmp"), "genes.bedGraph"), genes), "bedGraph lines")
