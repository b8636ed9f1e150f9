"""bamsignals_amd — MI355X-native interval counting with the interface of Bioconductor's bamsignals.

User API (mirrors R/wrappers.R and R/zzzCountSignals.R of the reference):
    bamCount, bamProfile, bamCoverage, CountSignals, GRanges, writeSamAsBamAndIndex
Beyond it: bamCrossCorr, the strand cross-correlation over ranges (the data's own value for ``shift``), and
bamFragSizes, the fragment-length histogram over ranges (the data's own ``tlenFilter``); bamDepthHist, the histogram of
the per-base depth over ranges (breadth at 20x, mean and median depth, the duplication histogram); bamSummary, every
range's own sum, max, summit and breadth at thresholds (peak heights, per-target QC); bamScaled, every range cut into
the same number of bins whatever its width (the heatmap matrix, metaprofiles over genes of unequal length); bamOverlaps,
the reads or fragments that overlap each range (countOverlaps / featureCounts / multicov counting); RunSignals, what
bamProfile / bamCoverage return with ``runs=True``: the signals as runs, encoded on the GPU; bamViews, the stretches of
every range at or above a depth with their sum, max and summit (callable regions, candidate peaks), found on the GPU;
bamVPlot, fragment length by position summed over ranges of one width (the V-plot of ATAC-seq, MNase and CUT&RUN around
TSSs, motif sites or dyads), made in one pass over the reads; bamJunctions, the splice junctions of every range with the reads
that support them and their largest anchor (summarizeJunctions, STAR's SJ.out.tab), counted on the GPU from the gap table of
the file's spliced reads; bamGeneCounts, the reads of every gene over its exons with the ambiguous, featureless, filtered and
unmapped reads beside them (htseq-count's union mode, featureCounts), each read decided on the GPU from the same spliced reads;
bamNucleotides, the A / C / G / T / N / deletion counts of every base of a range (Rsamtools::pileup, bam-readcount), counted
on the GPU from the bases and qualities the file's reads with bases keep; bamSites, the bases at which the reads disagree with
a reference or with each other (the candidate stage of VarScan and bcftools mpileup | call), judged on the GPU in the same
tiles so that only the sites come back.
Handle-level API for resident data and benchmarking: ``bamsignals_amd.device``.
All compute runs in hand-written HIP kernels for gfx950 behind the C ABI of
include/bamsignals_abi.h; there is no CPU fallback.
"""
from .bamio import BamFile, write_columns_as_bam, writeSamAsBamAndIndex  # noqa: F401
from .countsignals import CountSignals  # noqa: F401
from .crosscorr import CrossCorr, bamCrossCorr  # noqa: F401
from .depthhist import DepthHist, bamDepthHist  # noqa: F401
from .fragsizes import FragSizes, bamFragSizes  # noqa: F401
from .genecounts import GeneCounts, GeneModel, bamGeneCounts  # noqa: F401
from .granges import GRanges  # noqa: F401
from .junctions import Junctions, bamJunctions  # noqa: F401
from .nucleotides import NucleotideCounts, bamNucleotides  # noqa: F401
from .overlaps import bamOverlaps  # noqa: F401
from .runsignals import RunSignals  # noqa: F401
from .scaled import ScaledSignals, bamScaled  # noqa: F401
from .sites import AlleleSites, bamSites  # noqa: F401
from .summary import RangeSummary, bamSummary  # noqa: F401
from .views import SignalViews, bamViews  # noqa: F401
from .vplot import VPlot, bamVPlot  # noqa: F401
from .wrappers import bamCount, bamCoverage, bamProfile, coverage_core, pileup_core  # noqa: F401

__all__ = ["bamCount", "bamProfile", "bamCoverage", "bamCrossCorr", "CrossCorr", "bamFragSizes",
           "FragSizes", "bamDepthHist", "DepthHist", "bamSummary", "RangeSummary", "bamScaled", "ScaledSignals",
           "bamOverlaps", "bamViews", "SignalViews", "bamVPlot", "VPlot", "bamJunctions", "Junctions",
           "bamGeneCounts", "GeneCounts", "GeneModel", "bamNucleotides", "NucleotideCounts", "bamSites", "AlleleSites",
           "CountSignals", "RunSignals", "GRanges", "BamFile",
           "writeSamAsBamAndIndex", "write_columns_as_bam", "pileup_core", "coverage_core"]
