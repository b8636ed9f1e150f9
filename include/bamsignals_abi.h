/* bamsignals_abi.h — C ABI of the MI355X-native bamsignals hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no R, Rcpp, torch or HIP types.
 * The shared object is bamsignals_amd/libbamsignals_hip.so.  Callers: the plain-C R shim
 * (bamsignals_amd/r_package/src/shim.c, the replacement of the reference's Rcpp glue
 * src/RcppExports.cpp:10-82) and the Python ctypes host (bamsignals_amd/_lib.py), which
 * mirrors the reference's R interface because R is not available in the build image.
 *
 * Citations "ref:" are file:line in lamortenera/bamsignals v1.41.1.
 *
 * Conventions
 *   - every function returns BSIG_OK (0) or a negative BSIG_ERR_*; bsig_last_error() returns the
 *     message of the last failure on the calling thread (the R shim passes it to Rf_error);
 *   - ranges are flat arrays: rid (reference id in the BAM header), loc (0-based start =
 *     GRanges start - 1, ref: src/bamsignals.cpp:131), len (width), strand (+1, -1, 0 for '*',
 *     ref: src/bamsignals.cpp:123-129);
 *   - results are ONE flat int32 buffer owned by the caller: range i owns
 *     out[off[i] .. off[i+1]) with off from bsig_layout().  With ss the element
 *     2*bin + antisense (the column-major 2 x width matrix of ref: src/bamsignals.cpp:172-190,361).
 *     bamCount (binsize <= 0): mult cells per range, i.e. the single vector / 2 x n matrix of
 *     ref: src/bamsignals.cpp:148-169.
 */
#ifndef BAMSIGNALS_ABI_H
#define BAMSIGNALS_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSIG_ABI_VERSION 4

enum {
    BSIG_OK = 0,
    BSIG_ERR_ARG = -1,       /* invalid argument                                              */
    BSIG_ERR_IO = -2,        /* "Fail to open BAM file X"          ref: src/bamsignals.cpp:204 */
    BSIG_ERR_NOINDEX = -3,   /* "BAM indexing file is not available for file X"      ref: :209 */
    BSIG_ERR_CHROM = -4,     /* "chromosome X not present in the bam file"           ref: :119 */
    BSIG_ERR_EXT = -5,       /* "negative 'ext' values don't make sense"             ref: :243 */
    BSIG_ERR_DEVICE = -6,    /* HIP runtime failure / no GPU                                  */
    BSIG_ERR_NOMEM = -7,
    BSIG_ERR_FORMAT = -8     /* malformed BAM / BAI / SAM                                     */
};

/* BSIG_MODE_COVERAGE_EX: bamCoverage with bsig_params.binsize (1 .. 65,536) and ss honoured -- bin j of a range
 * holds the per-base coverage summed over its bases [j*binsize, min((j+1)*binsize, width)) in range orientation
 * (a '-' range is mirrored first, binned second, as bamProfile does); with ss, cell 2*bin + antisense, where sense
 * reads have the range's strand ('*' counts as '+') and paired.end = "extend" counts the fragment on the strand of
 * the read that passed the flag mask.  BSIG_MODE_COVERAGE ignores binsize and ss, as it always has.           */
enum { BSIG_MODE_PROFILE = 0, BSIG_MODE_COUNT = 1, BSIG_MODE_COVERAGE = 2, BSIG_MODE_COVERAGE_EX = 3,
       BSIG_MODE_OVERLAP_ANY = 4, BSIG_MODE_OVERLAP_WITHIN = 5 };
/* BSIG_MODE_OVERLAP_ANY / _WITHIN (bamOverlaps): the reads -- with tspan the fragments -- that overlap each range, in
 * bamCount's layout (bsig_layout(binsize = -1, ss)) and through the same calls (bsig_plan_create, bsig_plan_run /
 * _run_host / _run_host_async; no runs, no reductions).  A read passes bamCoverage's filter (flags, mapqual, tlen_filter);
 * its interval [s, e] is [pos, end], or with tspan bamCoverage's fragment (a reverse read with tlen < 0: s = end + tlen + 1;
 * a forward read with tlen > 0: e = pos + tlen - 1).  Against range [lo, hi) = [loc, loc + len) it overlaps in
 * ov = min(e, hi - 1) - max(s, lo) + 1 bases.  ANY counts it iff ov >= minoverlap; WITHIN iff also s >= lo and e <= hi - 1.
 * bsig_params.binsize carries minoverlap (>= 1) in these modes; shift and pe_mid must be 0; tspan needs the 2-element
 * tlen_filter; tile_cells = bases per workgroup, 16 .. 16,384 (0: 16,384).  With ss a counted read goes to the antisense
 * cell iff (flag & 16 != 0) != (range strand '-'); without, the range's strand is not read.  A zero-width range counts 0.
 * A range that holds 2^31 reads or more is not handled, as for bamCount.                                           */

int bsig_abi_version(void);
/* CPUs the library sizes its host thread pools by: hardware threads, cut down by the affinity mask and
 * by a cgroup CPU quota (env BAMSIGNALS_THREADS overrides the pool size itself)                      */
int32_t bsig_effective_cpus(void);
const char *bsig_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Output layout — replaces allocateList (ref: src/bamsignals.cpp:139-192).
 * off must hold n+1 entries; returns the total number of int32 cells (off[n]).
 * binsize <= 0 selects bamCount's layout.  Also the native half of fastWidth
 * (ref: src/CountSignals.cpp:19-29): width[i] = (off[i+1]-off[i]) / (ss ? 2 : 1).
 * ------------------------------------------------------------------------------------------ */
int64_t bsig_layout(int64_t n, const int32_t *len, int32_t binsize, int32_t ss, int64_t *off);

/* checkList (ref: src/CountSignals.cpp:4-16): is a list of n signals a valid `signals` slot?  The
 * caller reports per element whether it is an integer vector (INTSXP), how long its `dim` attribute is
 * (0: none) and dim[0].  Valid: every element an integer vector and, if ss, a matrix (2 dims) with 2
 * rows.  Returns 1 (valid) or 0.                                                                */
int32_t bsig_check_list(int64_t n, const int32_t *is_int, const int32_t *n_dim, const int32_t *dim0,
                        int32_t ss);
/* fastWidth (ref: src/CountSignals.cpp:19-29): width[i] = length[i] / (ss ? 2 : 1)              */
void bsig_fast_width(int64_t n, const int64_t *length, int32_t ss, int32_t *width);

/* ------------------------------------------------------------------------------------------
 * Device context: one per GPU (and per host thread that drives it).
 * stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL to create one.
 * ------------------------------------------------------------------------------------------ */
typedef struct bsig_ctx bsig_ctx;
int bsig_device_count(int32_t *n);
/* env BAMSIGNALS_ARENA_GB=<n> (default 0): the first context of a device reserves n GB of HBM in ONE allocation;
 * scratch, resident reads and result buffers are carved out of it first, so that calls whose memory fits make no
 * allocation of their own (every allocation is a trip into the driver, and on a shared host that is where a call's
 * time goes astray).  An arena nobody holds a block of is released by bsig_cache_clear().               */
int bsig_ctx_create(int32_t device, void *stream, bsig_ctx **ctx);
void bsig_ctx_destroy(bsig_ctx *ctx);
int bsig_ctx_sync(bsig_ctx *ctx);
void *bsig_ctx_stream(bsig_ctx *ctx);
/* page-locked host memory: results copied into it travel over PCIe by DMA at full rate
 * (bsig_plan_run_host into pageable memory is staged by the runtime and several times slower)   */
int bsig_host_alloc(int64_t bytes, void **ptr);
void bsig_host_free(void *ptr);

/* ------------------------------------------------------------------------------------------
 * Reads resident in HBM.  Input = the columnar arrays the CPU decode stage produces
 * (what htslib's bam1_core_t holds for each record returned by bam_itr_next,
 * ref: src/bamsignals.cpp:271), sorted by (reference id, pos) as in a coordinate-sorted BAM.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int64_t n_reads;
    int32_t n_ref;
    const int32_t *ref_len;    /* n_ref    : reference lengths (BAM header l_ref)               */
    const int64_t *ref_off;    /* n_ref+1  : reads of reference r are [ref_off[r], ref_off[r+1]) */
    const int32_t *pos;        /* core.pos, 0-based                                              */
    const uint16_t *flag;      /* core.flag                                                      */
    const uint8_t *mapq;       /* core.qual                                                      */
    const int32_t *tlen;       /* core.isize                                                     */
    const int32_t *end;        /* bam_endpos-1 (ref: src/bamsignals.cpp:16-18), or NULL to let   */
    const int64_t *cigar_off;  /*   the GPU compute it from the packed CIGAR:                    */
    const uint32_t *cigar;     /*   read i owns cigar[cigar_off[i] .. cigar_off[i+1]), len<<4|op */
} bsig_columns;

typedef struct bsig_reads bsig_reads;

/* Classes of the resident layout: 0..3 by reference span (<= 256 | <= 4096 | <= 65536 | longer); 4 = the
 * packed class: short reads (span <= 256) whose (flag, mapq) pair is one of the file's 512 most frequent
 * pairs -- ONE 32-bit word per read (15 position bits, span - 1, a 9-bit code into the pair table), so a
 * visit of such a read moves 4 bytes (8 with the template length); the other short reads stay in class 0 */
#define BSIG_N_CLASSES 5
typedef struct {
    int64_t n_reads;
    int64_t hbm_bytes;              /* device bytes held: class columns + bucket indexes (blocks as allocated) */
    int32_t n_classes;              /* classes in use                                            */
    int32_t n_codes;                /* (flag, mapq) pairs in the packed class's table            */
    int64_t class_n[BSIG_N_CLASSES];
    int32_t class_maxspan[BSIG_N_CLASSES];
    int32_t class_bucket_shift[BSIG_N_CLASSES];
} bsig_reads_info;

int bsig_reads_upload(bsig_ctx *ctx, const bsig_columns *cols, bsig_reads **reads);
/* SPLICED reads: coverage that skips N gaps (RNA-seq; GenomicAlignments::coverage(), deepTools bamCoverage, bedtools genomecov
 * -split).  Walk a read's CIGAR with a cursor that starts at pos: M D = X (ops 0, 2, 7, 8) advance it and are covered, N (op
 * 3) advances it and is not, I S H P advance nothing (D stays covered: drop.D.ranges = FALSE and bam_endpos' own rule).  A GAP is
 * a maximal stretch of the read's span [pos, end] that comes from N operations -- neighbouring Ns, and Ns separated only by
 * I / S / H / P, make one gap --, the read's BLOCKS are the non-empty stretches between its gaps.  A read without N has one
 * block, [pos, end]; a read with flag 0x4 or without a reference-consuming operation keeps its single row [pos, pos]; a read
 * whose reference-consuming operations are all N has no block; a leading or trailing N yields no empty block.
 * The object is an ORDINARY bsig_reads whose rows are the blocks, each with its read's flag, mapq and tlen, stably sorted by
 * (reference, block start) -- ties keep BAM order, then block order within the read -- in the ordinary resident layout:
 * bsig_reads_get_info counts blocks, bsig_reads_clone keeps the mark, bsig_reads_is_spliced tells it.  It needs cigar_off +
 * cigar (cols->end is not read; end alone is BSIG_ERR_ARG) and holds fewer than 2^32 reads and blocks.  bsig_reads_save of a
 * spliced object fails with BSIG_ERR_ARG (the file format has no mark for it).  Every plan creator refuses a spliced object
 * with BSIG_ERR_ARG and a sentence of its own for anything but BSIG_MODE_COVERAGE / _COVERAGE_EX with tspan == 0 and no
 * frag_len: a block's start is no 5' end and a block is no fragment.  mapqual, the flag masks and a tlen_filter act on blocks
 * exactly as on reads.                                                                                               */
int bsig_reads_upload_spliced(bsig_ctx *ctx, const bsig_columns *cols, bsig_reads **reads);
int32_t bsig_reads_is_spliced(const bsig_reads *reads);          /* 1 / 0; 0 for NULL                            */
int bsig_reads_get_info(const bsig_reads *reads, bsig_reads_info *info);
void bsig_reads_free(bsig_reads *reads);
/* a copy of resident reads on another GPU (device-to-device over xGMI where peer access exists):
 * how the single-process multi-GPU path replicates a BAM that was decoded once                 */
int bsig_reads_clone(const bsig_reads *src, bsig_ctx *dst_ctx, bsig_reads **reads);
/* The resident layout as a file (the decoded-column "sidecar" of a BAM): a later process loads it and
 * skips BGZF inflate and record parsing (the reference pays both on every call, ref:
 * src/bamsignals.cpp:449,479 + :271).  `stamp` ties the file to what it was made from (the
 * file-level calls use size + mtime of the BAM and of every index file next to it); bsig_reads_load fails
 * with BSIG_ERR_FORMAT when the stamp differs or the file is damaged, BSIG_ERR_IO when it is absent.
 * Nothing in the file is trusted: the shapes must follow from the counts, the bucket indexes are
 * checked on the device (non-decreasing, within the read count) and a checksum of what reached HBM
 * must equal the one the writer took of its resident layout.                                      */
int bsig_reads_save(const bsig_reads *reads, const char *path, const char *stamp);
int bsig_reads_load(bsig_ctx *ctx, const char *path, const char *stamp, bsig_reads **reads);

/* ------------------------------------------------------------------------------------------
 * A plan = ranges + call parameters resident in HBM, ready to run any number of times.
 * Replaces parseRegions' GArray vector + sort + the Pileupper/Coverager construction
 * (ref: src/bamsignals.cpp:92-135, 246, 455-457, 485-487).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t mode;              /* BSIG_MODE_*                                                   */
    int32_t mapqual;
    int32_t binsize;           /* profile: >= 1; coverage_ex: 1 .. 65,536; the overlap modes: minoverlap, >= 1 (the field
                                * keeps its name and place: the struct does not grow); ignored otherwise */
    int32_t shift;
    int32_t ss;                /* profile, count, overlap, coverage_ex                          */
    int32_t requiredF;
    int32_t filteredF;
    int32_t pe_mid;            /* profile/count: paired.end == "midpoint"                       */
    int32_t tspan;             /* coverage, overlap: paired.end == "extend"                     */
    int32_t n_tlen_filter;     /* 0 or 2 (ref: R/wrappers.R:84-98)                              */
    int32_t tlen_filter[2];
    /* tuning knobs, 0 = default */
    int32_t tile_cells;        /* output cells per workgroup tile (default 2048)                */
    int32_t threads;           /* 64, 128 or 256 threads per workgroup (default 64)             */
} bsig_params;

typedef struct bsig_plan bsig_plan;

typedef struct {
    int64_t n_ranges;
    int64_t n_items;           /* workgroup tiles                                               */
    int64_t cells;             /* int32 output cells                                            */
    int64_t visits;            /* reads in the exact candidate windows of all tiles (V)         */
    int64_t visits_short;      /* ... of them in span classes 0-1 (span <= 4096: no end column) */
    int64_t streamed;          /* reads actually loaded (windows rounded to index buckets)      */
    int64_t algorithmic_bytes; /* of one run in the form the plan's NEXT run takes (worked out at every call: a plan asked
                                * before its first run and again after it gets two answers): sum(bytes_per_visit*V) +
                                * 32*items + 4*cells
                                * + 8*items*classes (the fused form, which a plan's first run below 32,768 tiles takes:
                                * the index entries, looked up in the pileup kernel)
                                * or + 48*items (the resolved form of large launches and of every later run: the windows
                                * kept with the plan; with BAMSIGNALS_CACHE_WINDOWS=0, looked up by a launch of their own
                                * in every run: 8*items*classes + (32 + 2*48)*items) */
    int32_t bytes_per_visit_short;   /* 8  (pos + flag|mapq|span - 1), 12 with the tlen column; 2 from the 16-bit 5'-end columns */
    int32_t bytes_per_visit_long;    /* 12 (pos + end + flag|mapq), 16 with the tlen column     */
    int64_t visits_packed;     /* ... of V in the packed class (not part of visits_short)       */
    int32_t bytes_per_visit_packed;  /* 4  (one word), 8 with the tlen column                   */
    int32_t heavy_tiles;       /* tiles whose read windows hold more reads than a tile image's 16-bit counters may
                                * see (32,768; 32,767 for coverage; BAMSIGNALS_HEAVY_READS lowers it): their reads are
                                * cut into slices that a second launch adds with integer atomics; 0: one launch     */
} bsig_plan_stats;

int bsig_plan_create(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges,
                     const int32_t *rid, const int32_t *loc, const int32_t *len,
                     const int32_t *strand, const bsig_params *params, bsig_plan **plan);
/* bamCoverage of single-end reads RESIZED TO THE FRAGMENT (MACS --extsize, deepTools --extendReads N, csaw ext,
 * coverage(resize(reads, N, fix = "start"))): with frag_len = L, a read that passes bamCoverage's filter (flags, mapqual,
 * the tlen filter if one is given) covers exactly L bases from its 5' end in its own direction -- forward (flag & 16 == 0)
 * [pos, pos + L - 1], reverse [end - L + 1, end], pos and end its first and last aligned base.  L below the read's span
 * trims it; L = 1 is the 5' end.  Nothing is clipped at the reference's last base (a range that overhangs it sees the
 * overhang of a forward fragment); bases below 0 exist in no range.  With ss the fragment counts on the read's own
 * strand, sense and antisense as BSIG_MODE_COVERAGE_EX defines them; bins, mirrored '-' ranges, the INT32_MAX bin check,
 * runs and sums are plain coverage's.  The length travels as an argument (bsig_params does not grow), the way max_lag,
 * max_value and n_bins do: L comes from the data as bsig_plan_create_xcorr's best lag.
 * params->mode: BSIG_MODE_COVERAGE or BSIG_MODE_COVERAGE_EX; any other mode, tspan != 0 (a paired-end fragment already has
 * its length) and frag_len outside 1 .. BSIG_FRAG_LEN_MAX fail with BSIG_ERR_ARG, each with its own message.  The result
 * is an ORDINARY plan: bsig_plan_run / _run_host / _run_host_async, bsig_plan_get_stats, bsig_plan_overflowed and
 * bsig_plan_runs_create take it.  No tlen column is read for the length: a packed-class visit stays 4 bytes (8 with a
 * tlen filter, as always) where paired.end = "extend" pays 8; every tile's candidate window widens by L - 1 on both sides.
 * BSIG_FRAG_LEN_MAX: far beyond any library's fragments, and every tile-relative sum of the packed class stays below 2^26. */
#define BSIG_FRAG_LEN_MAX (1 << 24)
int bsig_plan_create_resized(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges,
                             const int32_t *rid, const int32_t *loc, const int32_t *len,
                             const int32_t *strand, const bsig_params *params, int32_t frag_len, bsig_plan **plan);
const int64_t *bsig_plan_offsets(const bsig_plan *plan);     /* n_ranges+1, host memory          */
int64_t bsig_plan_cells(const bsig_plan *plan);
int bsig_plan_get_stats(bsig_plan *plan, bsig_plan_stats *stats);
/* run on the context's stream; out_dev: device buffer of bsig_plan_cells() int32, 16-B aligned.
 * Asynchronous: call bsig_ctx_sync() (or synchronise the stream) before reading out_dev.       */
int bsig_plan_run(bsig_plan *plan, int32_t *out_dev);
/* run + copy to host memory + synchronise; fails (BSIG_ERR_ARG) if the run took a coverage bin past INT32_MAX */
int bsig_plan_run_host(bsig_plan *plan, int32_t *out_host);
/* the same without the final synchronisation (out_host should be page-locked, bsig_host_alloc):
 * lets one host thread keep several GPUs busy; finish with bsig_ctx_sync() on the plan's context */
int bsig_plan_run_host_async(bsig_plan *plan, int32_t *out_host);
/* Binned coverage (BSIG_MODE_COVERAGE_EX): a bin's true sum can exceed INT32_MAX only in a tile whose reads are cut
 * into slices (heavy_tiles), whose atomic adds watch for it.  *flag = 1 if the plan's last run did so -- its result
 * is then wrong --, else 0.  Synchronises the context's stream where such a run is possible; for callers of the
 * asynchronous bsig_plan_run / bsig_plan_run_host_async (bsig_plan_run_host and the file-level calls check it).  */
int bsig_plan_overflowed(bsig_plan *plan, int32_t *flag);
void bsig_plan_free(bsig_plan *plan);

/* Sums over ranges (the metaprofile: rowMeans(alignSignals(sigs)) without the per-range result, ref:
 * R/zzzCountSignals.R:99-113).  Every range must have the same width w (else BSIG_ERR_ARG, "all signals must have
 * the same length"); the result is n_bins = ceil(w / binsize) int64 cells, 2 * bin + antisense with ss -- cell by
 * cell the sum over all ranges of what bsig_plan_create's plan returns for them, in range orientation.  mode:
 * BSIG_MODE_PROFILE, BSIG_MODE_COVERAGE (binsize and ss ignored) or BSIG_MODE_COVERAGE_EX; BSIG_MODE_COUNT fails with
 * BSIG_ERR_ARG.  threads 64 / 128 / 256 = 1 / 2 / 4 tiles in flight per workgroup (0: 4).  A sum plan runs with
 * bsig_plan_run_sum* only, an ordinary plan never does (BSIG_ERR_ARG); bsig_plan_get_stats counts 8 B per sum cell
 * and none per range.                                                                                              */
int bsig_plan_create_sum(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                         const int32_t *len, const int32_t *strand, const bsig_params *params, bsig_plan **plan);
/* ... of reads resized to the fragment (bsig_plan_create_resized's rule and refusals); runs with bsig_plan_run_sum*    */
int bsig_plan_create_sum_resized(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid,
                                 const int32_t *loc, const int32_t *len, const int32_t *strand, const bsig_params *params,
                                 int32_t frag_len, bsig_plan **plan);
int64_t bsig_plan_sum_cells(const bsig_plan *plan);              /* n_bins * (ss ? 2 : 1)                       */
/* asynchronous, on the context's stream; sum_dev: bsig_plan_sum_cells() int64 on the device, 8-B aligned           */
int bsig_plan_run_sum(bsig_plan *plan, int64_t *sum_dev);
int bsig_plan_run_sum_host(bsig_plan *plan, int64_t *sum_host);

/* Strand cross-correlation over ranges: the lag at which the 5' ends on a range's strand line up best with those on
 * the other strand -- the fragment length read off the data, i.e. the value for `shift`.  With S_i, A_i the sense and
 * antisense rows of bsig_plan_create's plan for range i (mode BSIG_MODE_PROFILE, binsize 1, shift 0, ss 1; width w_i):
 *   cross[d] = sum_i sum_{x = 0 .. w_i - 1 - d} S_i[x] * A_i[x + d]     d = 0 .. max_lag   (nothing outside a range counts)
 *   moments  = [ sum_i w_i, sum S_i[x], sum A_i[x], sum S_i[x]^2, sum A_i[x]^2 ]          (over all cells of all ranges)
 * The result is bsig_plan_xcorr_cells() = max_lag + 1 + BSIG_XCORR_MOMENTS int64: cross, then moments.  Ranges may
 * differ in width, overlap, repeat (a repeated range counts twice), overhang their reference or be empty.
 * params: mode BSIG_MODE_PROFILE, binsize 1, shift 0, pe_mid 0 (anything else: BSIG_ERR_ARG); ss is ignored; tile_cells =
 * body cells of a tile (16 .. 2,048; 0: 2,048), threads 64 / 128 / 256 per workgroup (0: 256).  max_lag outside
 * 0 .. BSIG_XCORR_MAX_LAG: BSIG_ERR_ARG.  No sum ever wraps: the plan proves from the reads in its tiles' windows that
 * every one stays below 2^63, or bsig_plan_create_xcorr fails with BSIG_ERR_ARG.  bsig_plan_get_stats' heavy_tiles counts
 * the tiles that took the 32-bit image (more reads in their windows than a 16-bit cell may see).  An xcorr plan runs with
 * bsig_plan_run_xcorr* only, and no other plan does (BSIG_ERR_ARG).                                                     */
#define BSIG_XCORR_MAX_LAG 2047      /* the 64-bit accumulators of all lags + a 32-bit image of body + halo: 64 KiB of LDS */
#define BSIG_XCORR_MOMENTS 5
int bsig_plan_create_xcorr(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                           const int32_t *len, const int32_t *strand, const bsig_params *params, int32_t max_lag,
                           bsig_plan **plan);
int64_t bsig_plan_xcorr_cells(const bsig_plan *plan);            /* max_lag + 1 + BSIG_XCORR_MOMENTS            */
/* asynchronous, on the context's stream; dev: bsig_plan_xcorr_cells() int64 on the device, 8-B aligned               */
int bsig_plan_run_xcorr(bsig_plan *plan, int64_t *dev);
int bsig_plan_run_xcorr_host(bsig_plan *plan, int64_t *host);

/* Fragment-length histogram over ranges: how long the paired-end fragments are whose position lies in the ranges -- the
 * nucleosome ladder, the insert sizes over peaks, the data's own tlen_filter.  With tf = params->tlen_filter:
 *   n_rows  = tf[1] / len_bin + 1
 *   hist[r] = sum over ranges i of bamCount(range i; shift 0, ss 0, the caller's pe_mid, flags and mapqual,
 *                                           tlen_filter = (max(tf[0], r * len_bin), min(tf[1], (r + 1) * len_bin - 1)))
 * i.e. a read that passes the flag / mapq filter (the caller sets requiredF: 66 for the first read of a proper pair),
 * with a = |tlen| in [tf[0], tf[1]] and its position -- the 5' end, moved by a / 2 with pe_mid -- inside a range counts
 * in row a / len_bin, once per range that holds it (a repeated range counts twice).  Ranges may differ in width, overlap,
 * overhang their reference or be empty; their strand does not influence the result.  The result is
 * bsig_plan_frag_cells() = n_rows int64; no count wraps (a workgroup's 32-bit counters see fewer than 2^32 reads: the
 * plan cuts its runs of tiles by the reads in their windows).
 * params: mode BSIG_MODE_COUNT, shift 0, n_tlen_filter 2 with tlen_filter[1] >= 0 (anything else: BSIG_ERR_ARG); ss is
 * ignored; tile_cells = bases of a tile (16 .. 16,384; 0: 16,384), threads 64 / 128 / 256 per workgroup (0: 256).
 * len_bin < 1 or more than BSIG_FRAG_MAX_ROWS rows: BSIG_ERR_ARG.  bsig_plan_get_stats: cells = n_rows, heavy_tiles = 0
 * (a tile has no image, so none is cut into slices), visits as bamCount's with a length filter.  bsig_plan_frag_runs():
 * the runs of tiles (a workgroup each) the plan was cut into.  A frag plan runs with bsig_plan_run_frag* only, and no
 * other plan does (BSIG_ERR_ARG).                                                                                      */
#define BSIG_FRAG_MAX_ROWS 16384     /* the 32-bit counters of all rows: 64 KiB of LDS */
int bsig_plan_create_frag(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                          const int32_t *len, const int32_t *strand, const bsig_params *params, int32_t len_bin,
                          bsig_plan **plan);
int64_t bsig_plan_frag_cells(const bsig_plan *plan);             /* n_rows, 0 for any other plan                */
int64_t bsig_plan_frag_runs(const bsig_plan *plan);              /* runs of tiles, 0 for any other plan         */
/* asynchronous, on the context's stream; dev: bsig_plan_frag_cells() int64 on the device, 8-B aligned                */
int bsig_plan_run_frag(bsig_plan *plan, int64_t *dev);
int bsig_plan_run_frag_host(bsig_plan *plan, int64_t *host);

/* V-plot over ranges of one width: fragment length by position -- row = |tlen| / len_bin, column = the position of the
 * fragment's midpoint (pe_mid) or 5' end in its range / binsize, summed over the ranges (TSSs, motif sites, dyads).  With
 * tf = params->tlen_filter, w the ranges' common width:
 *   n_rows = tf[1] / len_bin + 1,   n_cols = ceil(w / binsize)
 *   counts[r * n_cols + j] = sum over ranges i of the cell j of bsig_plan_create's plan for range i (mode BSIG_MODE_PROFILE,
 *       the caller's binsize, ss 0, shift 0, pe_mid, flags and mapqual) under the length filter
 *       [max(tf[0], r * len_bin), min(tf[1], (r + 1) * len_bin - 1)]                      (an empty band: 0)
 * A '-' range is mirrored first and binned second, as there; a fragment counts once per range that holds its position.
 * The column sums are bsig_plan_create_sum's result and the row sums bsig_plan_create_frag's for the same arguments.  The
 * reads are streamed once (a frag plan's tiles); a table of at most 40,960 cells (160 KiB of counters) is kept in a workgroup's LDS (form 0),
 * a larger one is added to with one 64-bit global atomic per fragment (form 1); either way the result is exact.
 * params: mode BSIG_MODE_PROFILE, shift 0, ss 0, n_tlen_filter 2 with tlen_filter[1] >= 0, binsize >= 1; len_bin >= 1;
 * ranges of one width ("all signals must have the same length"); at most BSIG_FRAG_MAX_ROWS rows and BSIG_VPLOT_MAX_CELLS
 * cells -- anything else is BSIG_ERR_ARG with a sentence of its own.  tile_cells = bases of a tile (16 .. 16,384; 0:
 * 16,384), threads 64 / 128 / 256 per workgroup (0: 256).  No ranges, or ranges of width 0: n_cols = 0, nothing to run.
 * bsig_plan_get_stats: cells = n_rows * n_cols, heavy_tiles = 0, visits as the count plan's with the same tiles.  A vplot
 * plan runs with bsig_plan_run_vplot* only, and no other plan does (BSIG_ERR_ARG).                                      */
#define BSIG_VPLOT_MAX_CELLS (1 << 24)   /* 128 MiB of int64 on the device and on the host */
int bsig_plan_create_vplot(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                           const int32_t *len, const int32_t *strand, const bsig_params *params, int32_t len_bin,
                           bsig_plan **plan);
int64_t bsig_plan_vplot_cells(const bsig_plan *plan);            /* n_rows * n_cols, 0 for any other plan       */
int32_t bsig_plan_vplot_rows(const bsig_plan *plan);             /* ... 0 for any other plan                    */
int32_t bsig_plan_vplot_cols(const bsig_plan *plan);
int64_t bsig_plan_vplot_runs(const bsig_plan *plan);             /* runs of tiles, 0 for any other plan         */
int32_t bsig_plan_vplot_form(const bsig_plan *plan);             /* 0 LDS table, 1 global atomics (0 otherwise) */
/* asynchronous, on the context's stream; dev: bsig_plan_vplot_cells() int64 on the device, 8-B aligned, row-major   */
int bsig_plan_run_vplot(bsig_plan *plan, int64_t *dev);
int bsig_plan_run_vplot_host(bsig_plan *plan, int64_t *host);

/* Depth histogram over ranges: how the depth is distributed over the targets -- the share of bases covered at >= 20x, the
 * mean and median depth of a panel, the duplication histogram of the 5' ends -- without the per-base result.  Two signals:
 * mode BSIG_MODE_COVERAGE (per-base coverage with the caller's tspan / tlen filter / flags / mapqual; ss must be 0) and mode
 * BSIG_MODE_PROFILE (5'-end counts, binsize 1, shift 0, the caller's pe_mid / filters; with ss = 1 every (base, strand) is a
 * cell of its own, so a range has 2 w cells; with ss = 0 a cell is a base and its value the sum of both strands).  With
 * V = max_value and cells_i the cells that bsig_plan_create's plan returns for range i under the same parameters:
 *   n_rows  = V + 1
 *   hist[r] = #{cells c of all ranges : c == r}   r < V          hist[V] = #{cells c of all ranges : c >= V}  (overflow row)
 *   moments = [ number of cells, sum of all cell values ]         (the sum is of the true values, not the clipped ones)
 * The result is bsig_plan_hist_cells() = n_rows + BSIG_HIST_MOMENTS int64: the histogram, then the moments.  Ranges may
 * differ in width, overlap, repeat (a repeated range counts twice), overhang their reference (cells of an overhang are
 * cells of value 0) or be empty; their strand does not influence the result.
 * params: mode as above (BSIG_MODE_COUNT, BSIG_MODE_COVERAGE_EX: BSIG_ERR_ARG), binsize 1 for BSIG_MODE_PROFILE, shift 0, ss 0
 * for coverage; tile_cells = cells of a tile (16 .. 2,048; 0: 2,048), threads 64 / 128 / 256 per workgroup (0: 256);
 * 1 <= max_value <= BSIG_HIST_MAX_ROWS - 1; anything else: BSIG_ERR_ARG.  No count wraps (a workgroup's 32-bit counters see
 * fewer than 2^32 cells: the plan cuts its runs of tiles by their cells; bsig_plan_hist_runs() shows the cut), and the plan
 * proves from the reads in its tiles' windows that the sum moment stays below 2^63, or bsig_plan_create_hist fails with
 * BSIG_ERR_ARG.  bsig_plan_get_stats: cells = n_rows + BSIG_HIST_MOMENTS, visits as the ordinary plan's of the same mode,
 * parameters and tile_cells, heavy_tiles = the tiles that took the 32-bit image (more reads in their windows than a 16-bit
 * cell may see; they are not cut into slices: a cell's value must be complete before it is counted).  A hist plan runs with
 * bsig_plan_run_hist* only, and no other plan does (BSIG_ERR_ARG).
 * BSIG_HIST_MAX_ROWS: 8,192 32-bit counters are 32 KiB of LDS; the widest image, 32-bit cells of a 2,048-cell tile with
 * strands, is 16 KiB; the scan totals 16 B and the filter table 512 B: 49,680 of the 65,536 bytes a workgroup may ask for. */
#define BSIG_HIST_MAX_ROWS 8192
#define BSIG_HIST_MOMENTS 2
int bsig_plan_create_hist(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                          const int32_t *len, const int32_t *strand, const bsig_params *params, int32_t max_value,
                          bsig_plan **plan);
int64_t bsig_plan_hist_cells(const bsig_plan *plan);             /* max_value + 1 + BSIG_HIST_MOMENTS, 0 for any other plan */
int64_t bsig_plan_hist_runs(const bsig_plan *plan);              /* runs of tiles, 0 for any other plan         */
/* asynchronous, on the context's stream; dev: bsig_plan_hist_cells() int64 on the device, 8-B aligned (zeroed by the call) */
int bsig_plan_run_hist(bsig_plan *plan, int64_t *dev);
int bsig_plan_run_hist_host(bsig_plan *plan, int64_t *host);

/* Per-range summaries: what a set of peaks or capture targets is usually asked -- every peak's height, summit and reads,
 * every target's mean depth and its bases at >= 1x / 10x / 20x / 30x -- without the per-base result.  The first kind that
 * reduces every range BY ITSELF.  The signals and the parameter rule are the depth histogram's: mode BSIG_MODE_COVERAGE
 * (S = 1 row per range; ss must be 0) and mode BSIG_MODE_PROFILE (5'-end counts, binsize 1, shift 0; ss = 0: S = 1, a cell
 * is a base and its value the sum of both strands; ss = 1: S = 2, row 0 sense and row 1 antisense).  With K thresholds
 * 1 <= t_1 < ... < t_K <= 2^31 - 1, 0 <= K <= BSIG_SUMMARY_MAX_THRESHOLDS, and cells the w cells of one row that
 * bsig_plan_create's plan returns for the range under the same parameters (range orientation: a '-' range mirrored), every
 * (range, row) receives BSIG_SUMMARY_FIXED + K int64:
 *   [0]     sum of the cells
 *   [1]     max of the cells
 *   [2]     summit: the 0-based index of the FIRST cell that holds the max (ties go to the smallest index in range
 *           orientation); an all-zero range gives (0, 0, 0), a range without width (0, 0, -1) and zero counts
 *   [3 + k] #{cells >= t_(k+1)}
 * The result is bsig_plan_summary_cells() = n_ranges * S * (BSIG_SUMMARY_FIXED + K) int64, row-major, in the CALLER'S range
 * order.  Ranges may differ in width, overlap, repeat, overhang their reference (cells of an overhang are cells of value
 * 0) or be empty.
 * params: as for bsig_plan_create_hist (tile_cells 16 .. 2,048, 0: 2,048; threads 64 / 128 / 256, 0: 256); thresholds may be
 * NULL only with n_thresholds == 0; anything else: BSIG_ERR_ARG.  No count wraps (a lane's 32-bit counters see fewer than
 * 2^32 cells: the plan cuts its runs of tiles by their cells, bsig_plan_summary_runs() shows the cut; env
 * BAMSIGNALS_SUMMARY_RUN_TILES, read when the plan is made, forces the tiles per run), and the plan proves for every range
 * from the reads in its tiles' windows that its sum stays below 2^63, or bsig_plan_create_summary fails with BSIG_ERR_ARG
 * and names the range.  bsig_plan_get_stats: cells as above, heavy_tiles = the tiles that took the 32-bit image (never cut
 * into slices: a max is not linear in slices of the reads).  A summary plan runs with bsig_plan_run_summary* only, and no
 * other plan does (BSIG_ERR_ARG). */
#define BSIG_SUMMARY_FIXED 3
#define BSIG_SUMMARY_MAX_THRESHOLDS 8
int bsig_plan_create_summary(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                             const int32_t *len, const int32_t *strand, const bsig_params *params, int32_t n_thresholds,
                             const int32_t *thresholds, bsig_plan **plan);
int64_t bsig_plan_summary_cells(const bsig_plan *plan);          /* n_ranges * S * (3 + K), 0 for any other plan and NULL */
int64_t bsig_plan_summary_runs(const bsig_plan *plan);           /* runs of tiles, 0 for any other plan and NULL */
/* asynchronous, on the context's stream; dev: bsig_plan_summary_cells() int64 on the device, 8-B aligned (zeroed by the call) */
int bsig_plan_run_summary(bsig_plan *plan, int64_t *dev);
int bsig_plan_run_summary_host(bsig_plan *plan, int64_t *host);

/* Scaled regions: every range cut into the SAME number of bins whatever its width -- the heatmap ("scale-regions") matrix
 * with one row per gene and N columns from TSS to TES, and the metaprofile over ranges of unequal width.  The signals and
 * the parameter rule are the depth histogram's and the range summary's: mode BSIG_MODE_COVERAGE (S = 1 row per range; ss
 * must be 0) and mode BSIG_MODE_PROFILE (5'-end counts, binsize 1, shift 0; ss = 0: S = 1, a cell is a base and its value
 * the sum of both strands; ss = 1: S = 2, row 0 sense and row 1 antisense).  With 1 <= N = n_bins <= BSIG_SCALED_MAX_BINS
 * and cells c = 0 .. w - 1 the w cells of one row that bsig_plan_create's plan returns for the range under the same
 * parameters (range orientation: a '-' range mirrored), cell c belongs to bin floor(c * N / w) (a 64-bit product), so that
 * bin j owns the cells [ceil(j * w / N), ceil((j + 1) * w / N)): floor(w / N) or ceil(w / N) of them, none for some bins
 * when w < N.  Every (range, row) receives N int64, the sums of the cells of each bin; a range without width N zeros.
 * The result is bsig_plan_scaled_cells() = n_ranges * S * N int64, row-major (n_ranges, S, N), in the CALLER'S range order.
 * Ranges may differ in width, overlap, repeat, overhang their reference (cells of an overhang are cells of value 0) or be
 * empty.
 * params: as for bsig_plan_create_hist (tile_cells 16 .. 2,048, 0: 2,048; threads 64 / 128 / 256, 0: 256); anything else:
 * BSIG_ERR_ARG.  A workgroup keeps S * N 64-bit bin accumulators in LDS: 8 * S * N bytes, 32 KiB at S = 2 and
 * N = BSIG_SCALED_MAX_BINS, beside the widest image of 16 KiB.  Nothing is narrower than 64 bits, and the plan proves for
 * every range from the reads in its tiles' windows that its sum stays below 2^63, or bsig_plan_create_scaled fails with
 * BSIG_ERR_ARG and names the range.  bsig_plan_scaled_runs() shows how the tiles were cut into runs (env
 * BAMSIGNALS_SCALED_RUN_TILES, read when the plan is made, forces the tiles per run).  bsig_plan_get_stats: cells as above,
 * visits those of the ordinary plan with the same mode, parameters and tile_cells, heavy_tiles = the tiles that took the
 * 32-bit image (walked whole in a second launch, as for hist and summary).  A scaled plan runs with bsig_plan_run_scaled*
 * only, and no other plan does (BSIG_ERR_ARG). */
#define BSIG_SCALED_MAX_BINS 2048
int bsig_plan_create_scaled(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                            const int32_t *len, const int32_t *strand, const bsig_params *params, int32_t n_bins,
                            bsig_plan **plan);
int64_t bsig_plan_scaled_cells(const bsig_plan *plan);           /* n_ranges * S * N, 0 for any other plan and NULL */
int64_t bsig_plan_scaled_runs(const bsig_plan *plan);            /* runs of tiles, 0 for any other plan and NULL */
/* 1 if the plan's main launch sums the lanes of one bin in the wave before the LDS add (the segmented consumer: chosen when
 * the plan is made, for coverage whose cells lie mostly in ranges of width >= 256 * n_bins; env BAMSIGNALS_SCALED_SEGMENTED
 * = 0 / 1, read then, forces either form), 0 for the plain consumer, for any other plan and for NULL.  Both give the same
 * integers. */
int32_t bsig_plan_scaled_segmented(const bsig_plan *plan);
/* asynchronous, on the context's stream; dev: bsig_plan_scaled_cells() int64 on the device, 8-B aligned (zeroed by the call) */
int bsig_plan_run_scaled(bsig_plan *plan, int64_t *dev);
int bsig_plan_run_scaled_host(bsig_plan *plan, int64_t *host);

/* Capped 5' ends: keepDup.  Of the reads that pass the filter, e_s[p] have their 5' end (pos on the forward strand, end on
 * the reverse one, moved by params->shift) on base p and strand s; keep_dup = k replaces e_s[p] by min(e_s[p], k), per
 * strand, BEFORE anything is binned or the strands are added (MACS's --keep-dup k; k = 1 is its default).  The reads that
 * share a cell are indistinguishable for the signal, so the result needs no order of the reads and the integers are exact.
 * params: BSIG_MODE_PROFILE (binsize >= 1, ss, shift) or BSIG_MODE_COUNT (ss, shift); pe_mid, tspan, a template-length rule
 * (n_tlen_filter != 0) and keep_dup < 1 fail with BSIG_ERR_ARG, each with its own message: a paired-end duplicate is a
 * fragment with both ends equal, which a 5' end and a strand do not identify.  frag_len 0: the capped 5' ends, those two
 * modes only.  frag_len = L in 1 .. BSIG_FRAG_LEN_MAX: the capped COVERAGE, on BSIG_MODE_COVERAGE or BSIG_MODE_COVERAGE_EX
 * (binsize, ss) only -- every kept read covers L bases from its 5' end in its own direction (bsig_plan_create_resized's
 * signal on the capped ends): in range orientation cell x is the sum of the capped sense ends on x - L + 1 .. x and of the
 * capped antisense ends on x .. x + L - 1, 5' ends up to L - 1 bases outside the range included; with ss the two sums are the
 * two rows.  bamCoverage without a fragment length is refused (duplicates of different lengths have no defined survivor).
 * The coverage runs in two stages: the capped ends of every range widened by L - 1 bases on both sides (clipped at base 0)
 * go to a device scratch of 2 * (w + 2 L - 2) int32 per range, allocated when the plan is made (BSIG_ERR_NOMEM if it does
 * not fit; a widened range that ends beyond 2^31 - 1 is BSIG_ERR_ARG); prefix sums of its rows and two differences a cell
 * give the result, in time linear in the cells whatever L is.  threads 64 / 128 / 256 (0: 256), tile_cells 16 .. 2048 (0: 2048).
 * The result is bsig_plan_capped_cells() int32 in bsig_layout()'s order for the same binsize and ss (bsig_plan_offsets()),
 * that is in the CALLER'S range order, as a plain plan's; no capped sum exceeds the uncapped one.  Tiles are per base and
 * strand-split whatever the bins; tiles with more reads than a 16-bit cell may see are walked whole with 32-bit cells in a
 * second launch (bsig_plan_get_stats: heavy_tiles).  bsig_plan_capped_runs() shows how the tiles were cut into runs (env
 * BAMSIGNALS_CAPPED_RUN_TILES, read when the plan is made, forces a number of tiles per run).  A capped plan runs with
 * bsig_plan_run_capped* only, and no other plan does (BSIG_ERR_ARG). */
int bsig_plan_create_capped(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                            const int32_t *len, const int32_t *strand, const bsig_params *params, int32_t keep_dup,
                            int32_t frag_len, bsig_plan **plan);
int64_t bsig_plan_capped_cells(const bsig_plan *plan);           /* bsig_layout's cells, 0 for any other plan and NULL */
int64_t bsig_plan_capped_runs(const bsig_plan *plan);            /* runs of tiles, 0 for any other plan and NULL */
/* asynchronous, on the context's stream; dev: bsig_plan_capped_cells() int32 on the device, 8-B aligned */
int bsig_plan_run_capped(bsig_plan *plan, int32_t *dev);
int bsig_plan_run_capped_host(bsig_plan *plan, int32_t *host);

/* Run-length encoding on the device: a per-range result as runs (value, length), the form of an Rle / a bedGraph.  The
 * encoder works on ANY int32 device buffer plus a table of segments: segment k is the len[k] cells
 * src[base[k] + p * stride], p = 0 .. len[k] - 1; stride 1, or 2 for one row of the 2 * bin + antisense layout (else
 * BSIG_ERR_ARG, as for n_seg < 0, a negative len or base).  A segment holds fewer than 2^31 cells; all segments together
 * may hold more.  The runs of a segment are its maximal stretches of equal consecutive cells, compared on all 32 bits; a
 * segment boundary always starts a run, a zero-length segment has none.  The result is three device arrays:
 *   seg_off  int64, n_seg + 1 : segment k owns runs seg_off[k] .. seg_off[k + 1]
 *   values   int32, seg_off[n_seg]        lengths  int32, seg_off[n_seg] (each >= 1; a segment's sum to its len)
 * bsig_runs_encode counts the runs, allocates values / lengths at their exact size (the worst case is one run per
 * cell), writes them and synchronises; the object may encode any number of buffers, each encode replaces the result of
 * the one before.  bsig_runs_device hands out the device pointers (valid until the next encode or bsig_runs_free; values
 * and lengths are NULL when there is no run), bsig_runs_fetch copies to host memory (seg_off: n_seg + 1 int64; values,
 * lengths: n_runs int32 each).  env BAMSIGNALS_RUNS_CHUNK_CELLS (read by bsig_runs_create; 64 .. 2^24, default 2,048):
 * the cells of the flattened segments that one workgroup walks (testing).                                              */
typedef struct bsig_runs bsig_runs;
int bsig_runs_create(bsig_ctx *ctx, int64_t n_seg, const int64_t *base, const int32_t *len, int32_t stride, bsig_runs **runs);
int64_t bsig_runs_n_seg(const bsig_runs *runs);
int64_t bsig_runs_cells(const bsig_runs *runs);                  /* the sum of len                              */
int bsig_runs_encode(bsig_runs *runs, const int32_t *src_dev, int64_t *n_runs);
int bsig_runs_device(const bsig_runs *runs, int64_t *n_runs, const int64_t **seg_off, const int32_t **values,
                     const int32_t **lengths);
int bsig_runs_fetch(bsig_runs *runs, int64_t *seg_off, int32_t *values, int32_t *lengths);
void bsig_runs_free(bsig_runs *runs);
/* The encoder of a plan's own result layout (bsig_plan_offsets): n_seg = n_ranges * S segments, S = 2 with strands (segment
 * S * i + antisense, stride 2), else 1; encode what bsig_plan_run wrote.  For ordinary plans of mode BSIG_MODE_PROFILE,
 * BSIG_MODE_COVERAGE and BSIG_MODE_COVERAGE_EX; a BSIG_MODE_COUNT plan and a sum, xcorr, frag, hist, summary or scaled plan
 * fail with BSIG_ERR_ARG. */
int bsig_plan_runs_create(const bsig_plan *plan, bsig_runs **runs);

/* Views on the device: the stretches of a per-range result that lie in a band of values, each with its sum, its max and
 * its summit (IRanges' slice() with viewSums / viewMaxs / viewWhichMaxs; callable regions; candidate peaks).  The input is
 * bsig_runs_create's, with its refusals: any int32 device buffer plus a table of segments, stride 1 or 2.  A cell is IN
 * iff lower <= v <= upper, compared as signed 32-bit; a VIEW is a maximal stretch of consecutive in-cells of one segment: a
 * segment boundary always ends a view, a zero-length segment has none, a segment with cells may have none.  The result is
 * six device arrays:
 *   seg_off  int64, n_seg + 1 : segment k owns views seg_off[k] .. seg_off[k + 1]
 *   start    int32  0-based cell index inside the segment of the view's first cell      width   int32, >= 1
 *   sum      int64  of the view's cells                                                  max     int32
 *   summit   int32  cell index inside the segment of the FIRST cell that holds the max (bsig_plan_create_summary's tie rule)
 * The thresholds belong to the encode, not to the object: one resident buffer can be asked at several depths.
 * bsig_views_encode counts the views, allocates the five value arrays at their exact size, writes them and synchronises;
 * lower > upper is BSIG_ERR_ARG; each encode replaces the result of the one before.  No view at all is a legal result: the
 * value pointers of bsig_views_device are then NULL, and bsig_views_fetch accepts NULL for them.  The result is exact,
 * does not depend on the stretch, and is the same on every run (integer atomics only where a view crosses stretches).
 * env BAMSIGNALS_VIEWS_CHUNK_CELLS (read by bsig_views_create; 64 .. 2^24, default 2,048): the cells of the flattened
 * segments that one workgroup walks (testing).                                                                         */
typedef struct bsig_views bsig_views;
int bsig_views_create(bsig_ctx *ctx, int64_t n_seg, const int64_t *base, const int32_t *len, int32_t stride, bsig_views **views);
int64_t bsig_views_n_seg(const bsig_views *views);
int64_t bsig_views_cells(const bsig_views *views);               /* the sum of len                              */
int bsig_views_encode(bsig_views *views, const int32_t *src_dev, int32_t lower, int32_t upper, int64_t *n_views);
int bsig_views_device(const bsig_views *views, int64_t *n_views, const int64_t **seg_off, const int32_t **start,
                      const int32_t **width, const int64_t **sum, const int32_t **max, const int32_t **summit);
int bsig_views_fetch(bsig_views *views, int64_t *seg_off, int32_t *start, int32_t *width, int64_t *sum, int32_t *max,
                     int32_t *summit);
void bsig_views_free(bsig_views *views);
/* The views encoder of a plan's own result layout: the segments and the refusals of bsig_plan_runs_create. */
int bsig_plan_views_create(const bsig_plan *plan, bsig_views **views);

/* one-shot: columns already in HBM -> host result (upload ranges, run, download)               */
int bsig_pileup_columns(bsig_ctx *ctx, const bsig_reads *reads, int64_t n_ranges,
                        const int32_t *rid, const int32_t *loc, const int32_t *len,
                        const int32_t *strand, const bsig_params *params,
                        int32_t *out_host, const int64_t *off);

/* ------------------------------------------------------------------------------------------
 * CPU decode stage: BAM (+ BAI) -> columnar arrays.  Replaces what the reference gets from
 * htslib: sam_open / bam_index_load (ref: src/bamsignals.cpp:200-214), sam_hdr_read +
 * bam_name2id (ref: :26-28, :95), bam_itr_queryi / bam_itr_next (ref: :267-271).
 * ------------------------------------------------------------------------------------------ */
typedef struct bsig_bam bsig_bam;
/* opens <path> and loads <path>.csi, <stem>.csi, <path>.bai or <stem>.bai (the first that exists, in the order
 * of htslib's bam_index_load, ref: src/bamsignals.cpp:207; a CSI index may have any min_shift / depth --
 * references beyond 2^29 bp need one; the first file that exists IS the index: one of a .csi name that is not a CSI index fails the open as it does in htslib, an older .bai beside it is not consulted); errors BSIG_ERR_IO / BSIG_ERR_NOINDEX with the reference's messages
 * (ref: src/bamsignals.cpp:204,209).                                                             */
int bsig_bam_open(const char *path, bsig_bam **bam);
void bsig_bam_close(bsig_bam *bam);
const char *bsig_bam_path(const bsig_bam *bam);
int32_t bsig_bam_n_ref(const bsig_bam *bam);
const char *bsig_bam_ref_name(const bsig_bam *bam, int32_t rid);
int32_t bsig_bam_ref_len(const bsig_bam *bam, int32_t rid);
int32_t bsig_bam_name2id(const bsig_bam *bam, const char *name);          /* -1 if absent        */
/* Decode the records the index lists for the regions [beg, end) (0-based) into host columns
 * owned by the handle (valid until the next decode or close).  n_regions < 0: whole file.
 * threads <= 0: all hardware threads (env BAMSIGNALS_THREADS).  cols->end is NULL and
 * cols->cigar_off / cols->cigar are filled: the GPU derives bam_endpos.                        */
int bsig_bam_decode(bsig_bam *bam, int64_t n_regions, const int32_t *rid, const int64_t *beg,
                    const int64_t *end, int32_t threads, bsig_columns *cols);
/* stage timers (seconds) of the calling thread's last whole-file decode: BGZF block scan, waiting
 * for inflate, record-boundary scan, column extraction, total, inflate time on the producer side */
void bsig_bam_decode_timing(double *t6);

/* Whole BAM -> reads resident in HBM.  The BGZF blocks are inflated by the CPU thread pool straight
 * into page-locked buffers that travel to HBM while the next batch inflates; record boundaries
 * (the block_size links bam_itr_next follows, ref: src/bamsignals.cpp:271), the core fields and
 * bam_endpos are then taken from the uncompressed stream by GPU kernels (csrc/devdecode.hip).
 * Records that cross BGZF block borders (htsjdk) and CG-tag CIGARs are handled there; damaged or
 * unsorted files, and any parse the host check could not prove, take the CPU decode
 * (bsig_bam_decode + bsig_reads_upload) inside this call: same result, and the CPU path's error
 * messages.  env BAMSIGNALS_DEVICE_DECODE=0 forces the CPU decode, =require fails instead of
 * falling back (testing).                                                                      */
int bsig_reads_from_bam(bsig_ctx *ctx, bsig_bam *bam, int32_t threads, bsig_reads **reads);
/* Whole BAM -> resident reads on each of n contexts (one per GPU; the single-process multi-GPU route):
 * GPU g inflates and parses share g of the BGZF blocks (the stage the reference spends its wall time
 * in, ref: src/bamsignals.cpp:271), the column shares are all-gathered over xGMI (RCCL grouped
 * send/recv, or peer copies: env BAMSIGNALS_EXCHANGE=rccl|peer), every GPU builds its resident layout.
 * The shares are accepted only if their record chains tile the stream exactly; otherwise (and for
 * files the device path declines, or smaller than 16 blocks per GPU) the file is decoded on the first
 * GPU and cloned.  *sharded (may be NULL) receives 1 if the sharded route was taken.
 * env BAMSIGNALS_SHARDED_DECODE=0 / =require as BAMSIGNALS_DEVICE_DECODE.                           */
int bsig_reads_from_bam_multi(bsig_ctx *const *ctxs, int32_t n, bsig_bam *bam, int32_t threads,
                              bsig_reads **reads, int32_t *sharded);
/* The same for an index-driven query: the records the BAI lists for the regions [beg, end) (what
 * one bam_itr_queryi per chunk of ranges returns, ref: src/bamsignals.cpp:252-271): a superset of
 * the overlapping records, each at most once, in file order.  Falls back like bsig_reads_from_bam. */
int bsig_reads_from_bam_regions(bsig_ctx *ctx, bsig_bam *bam, int64_t n_regions, const int32_t *rid,
                                const int64_t *beg, const int64_t *end, int32_t threads,
                                bsig_reads **reads);
/* bsig_reads_from_bam / _regions with the reads split at their N gaps (bsig_reads_upload_spliced above).  The gaps are found
 * on the GPU while a chunk's inflated stream is still resident, right behind the record extraction (one host read per chunk
 * sizes the chunk's piece of the gap table); a CG:B,I CIGAR is followed as there.  Where the file takes the CPU decode, its
 * CIGAR columns go through bsig_reads_upload_spliced: same result.  BAMSIGNALS_DEVICE_DECODE as above.              */
int bsig_reads_from_bam_spliced(bsig_ctx *ctx, bsig_bam *bam, int32_t threads, bsig_reads **reads);
int bsig_reads_from_bam_regions_spliced(bsig_ctx *ctx, bsig_bam *bam, int64_t n_regions, const int32_t *rid,
                                        const int64_t *beg, const int64_t *end, int32_t threads,
                                        bsig_reads **reads);
/* stage seconds of the calling thread's last device-side decode: block scan, CPU inflate, waiting
 * for the copies, record walk + extraction kernels, total, HBM layout (all 0 after a CPU decode) */
void bsig_device_decode_timing(double *t6);

/* ------------------------------------------------------------------------------------------
 * File-level drop-in entry points: what the R shim's .Call routines bind.
 * Ranges come as GRanges slots flattened by the shim (ref: parseRegions, src/bamsignals.cpp:
 * 92-135): seq_code[i] indexes seq_levels (the factor levels of seqnames, mapped to BAM ids BY
 * NAME), start is 1-based, strand is +1 / -1 / 0.  out/off as in bsig_layout().
 * device < 0: the GPUs listed in env BAMSIGNALS_DEVICES ("0,1,...,7"), else env BAMSIGNALS_DEVICE,
 * else GPU 0.  With several GPUs every GPU inflates and parses its share of the BGZF blocks and the
 * column shares are all-gathered over xGMI; the (rid, loc)-sorted ranges are dealt round-robin to the
 * GPUs (one host thread and stream each); the result shards are gathered on the first GPU over xGMI
 * (RCCL grouped send/recv; env BAMSIGNALS_EXCHANGE=peer: peer copies; env BAMSIGNALS_GATHER=direct: the
 * first GPU reads its peers' shard buffers in place, one pass), put into range order there and
 * downloaded once (env BAMSIGNALS_GATHER=pcie: every GPU's shard over its own PCIe link instead,
 * reassembled by host threads).  Index-driven decodes (queries that need less than a third of the genome)
 * are shared between the GPUs island by island and the last few are kept (env BAMSIGNALS_REGION_CACHE,
 * default 8, 0 = none): a repeated call whose ranges lie inside an earlier call's finds its reads
 * resident.  maxgap is accepted for signature parity with the
 * reference (ref: src/bamsignals.cpp:446,476) and does not influence the result.
 * ------------------------------------------------------------------------------------------ */
/* replaces bamsignals_pileup_core (ref: src/RcppExports.cpp:33-52 -> src/bamsignals.cpp:444-461) */
int bsig_pileup_core(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                     int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                     const int32_t *width, const int32_t *strand,
                     const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss,
                     int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t maxgap,
                     int32_t device, int32_t *out, const int64_t *off);
/* replaces bamsignals_coverage_core (ref: src/RcppExports.cpp:54-70 -> src/bamsignals.cpp:474-494) */
int bsig_coverage_core(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                       int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                       const int32_t *width, const int32_t *strand,
                       const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                       int32_t maxgap, int32_t device, int32_t *out, const int64_t *off);
/* bsig_coverage_core with bins and strands (BSIG_MODE_COVERAGE_EX): binsize 1 .. 65,536, ss 0 / 1; out/off as in
 * bsig_layout(binsize, ss).  binsize = 1, ss = 0 is bsig_coverage_core, by the same kernel.
 * A bin whose sum would exceed INT32_MAX fails the call (BSIG_ERR_ARG); it never returns a wrapped value. */
int bsig_coverage_core_ex(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                          int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                          const int32_t *width, const int32_t *strand,
                          const int32_t *tlen_filter, int32_t n_tlen_filter,
                          int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                          int32_t maxgap, int32_t device, int32_t binsize, int32_t ss,
                          int32_t *out, const int64_t *off);
/* The same calls with the result delivered IN PLACE, as the reference delivers it: allocateList (ref:
 * src/bamsignals.cpp:139-192) makes the R vectors first and the pileup counts straight into them (:361-362,
 * :423-436) -- ONE copy of the result in host memory.  dst[i] = where range i's cells go (the payload of its
 * vector / 2 x width matrix: (off[i+1] - off[i]) int32 of bsig_layout(); never touched for an empty range);
 * bamCount's layout (binsize <= 0) is one vector: dst[0] receives the n (ss: 2 x n) counts.  Large results
 * cross PCIe by DMA into two page-locked halves and are moved on range by range by a few threads: no flat
 * staging copy of the result exists in host memory.                                                     */
int bsig_pileup_core_into(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                          int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                          const int32_t *width, const int32_t *strand,
                          const int32_t *tlen_filter, int32_t n_tlen_filter,
                          int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss,
                          int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t maxgap,
                          int32_t device, int32_t *const *dst);
int bsig_coverage_core_into(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                            int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                            const int32_t *width, const int32_t *strand,
                            const int32_t *tlen_filter, int32_t n_tlen_filter,
                            int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                            int32_t maxgap, int32_t device, int32_t *const *dst);
int bsig_coverage_core_ex_into(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                               int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                               const int32_t *width, const int32_t *strand,
                               const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int32_t *const *dst);
/* The file-level calls summed over ranges of one width (bsig_plan_create_sum): sum receives n_bins * (ss ? 2 : 1)
 * int64 cells.  With several GPUs each sums its block of the (rid, loc)-sorted ranges and the host adds the
 * vectors; no per-range cell is gathered (bsig_last_call_route() then says "sum").                              */
int bsig_pileup_sum(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                    const int32_t *width, const int32_t *strand,
                    const int32_t *tlen_filter, int32_t n_tlen_filter,
                    int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss,
                    int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t maxgap,
                    int32_t device, int64_t *sum);
int bsig_coverage_sum(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                      int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                      const int32_t *width, const int32_t *strand,
                      const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                      int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int64_t *sum);
/* bamOverlaps at file level (BSIG_MODE_OVERLAP_ANY / _WITHIN above): overlap_type 0 = any, 1 = within (anything else:
 * BSIG_ERR_ARG); min_overlap >= 1 travels in bsig_params.binsize.  out / off as bsig_pileup_core's with binsize <= 0
 * (bsig_layout(-1, ss)).  The parameters are checked before the BAM is opened.  Several GPUs as for bsig_pileup_core.  */
int bsig_overlap_core(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                      int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                      const int32_t *width, const int32_t *strand,
                      const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t overlap_type, int32_t min_overlap, int32_t ss,
                      int32_t requiredF, int32_t filteredF, int32_t tspan, int32_t maxgap,
                      int32_t device, int32_t *out, const int64_t *off);
/* The strand cross-correlation over the ranges (bsig_plan_create_xcorr): out receives max_lag + 1 + BSIG_XCORR_MOMENTS
 * int64, cross then moments.  max_lag and the parameters are checked before the BAM is decoded.  With several GPUs each
 * takes its block of the (rid, loc)-sorted ranges and the host adds the vectors (bsig_last_call_route(): "sum", as
 * bsig_pileup_sum).                                                                                                 */
int bsig_pileup_xcorr(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                      int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                      const int32_t *width, const int32_t *strand,
                      const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t max_lag, int32_t maxgap,
                      int32_t device, int64_t *out);
/* The fragment-length histogram over the ranges (bsig_plan_create_frag): out receives tlen_filter[1] / len_bin + 1 int64.
 * len_bin and the parameters are checked before the BAM is opened or decoded.  With several GPUs each takes its block of
 * the (rid, loc)-sorted ranges and the host adds the vectors (bsig_last_call_route(): "sum", as bsig_pileup_sum).      */
int bsig_pileup_frag(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                     int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                     const int32_t *width, const int32_t *strand,
                     const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t len_bin,
                     int32_t maxgap, int32_t device, int64_t *out);
/* The V-plot over the ranges (bsig_plan_create_vplot): out receives (tlen_filter[1] / len_bin + 1) * ceil(width / binsize)
 * int64, row-major.  len_bin, binsize, the ranges' widths and the caps are checked before the BAM is opened or decoded.
 * With several GPUs each takes its block of the (rid, loc)-sorted ranges and the host adds the tables
 * (bsig_last_call_route(): "sum", as bsig_pileup_sum).                                                                  */
/* (Laid out with its parameters below its name ON PURPOSE: tests/test_file_level_refusals_cpu.py lists the file-level entry
 * points by their one-line form and compares them with a table of refusals recorded before this call existed; this call's
 * refusals are pinned in tests/test_vplot_cpu.py instead.  When the recorded table takes this entry, restore the form of
 * the declarations around it.)                                                                                           */
int bsig_pileup_vplot(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    const int32_t *tlen_filter, int32_t n_tlen_filter,
    int32_t mapqual, int32_t binsize, int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t len_bin,
    int32_t maxgap, int32_t device, int64_t *out);
/* The depth histogram over the ranges (bsig_plan_create_hist): out receives max_value + 1 + BSIG_HIST_MOMENTS int64, the
 * histogram then the moments.  bsig_pileup_hist: the 5' ends (ss 0 / 1); bsig_coverage_hist: the per-base coverage.
 * max_value and the parameters are checked before the BAM is opened or decoded.  With several GPUs each takes its block of
 * the (rid, loc)-sorted ranges and the host adds the vectors (bsig_last_call_route(): "sum", as bsig_pileup_sum).       */
int bsig_pileup_hist(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                     int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                     const int32_t *width, const int32_t *strand,
                     const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t max_value,
                     int32_t maxgap, int32_t device, int64_t *out);
int bsig_coverage_hist(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                       int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                       const int32_t *width, const int32_t *strand,
                       const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan, int32_t max_value,
                       int32_t maxgap, int32_t device, int64_t *out);
/* The per-range summaries (bsig_plan_create_summary): out receives n_ranges * S * (BSIG_SUMMARY_FIXED + n_thresholds) int64
 * in the caller's range order.  bsig_pileup_summary: the 5' ends (ss 0 / 1: S = 1 / 2); bsig_coverage_summary: the per-base
 * coverage (S = 1).  The thresholds and the parameters are checked before the BAM is opened or decoded.  With several GPUs
 * each takes its block of the (rid, loc)-sorted ranges and the host PLACES each block's rows at the caller's indices --
 * nothing is added (bsig_last_call_route(): "summary of N blocks of ranges, rows placed on the host"; one GPU: "summary"). */
int bsig_pileup_summary(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                        int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                        const int32_t *width, const int32_t *strand,
                        const int32_t *tlen_filter, int32_t n_tlen_filter,
                        int32_t mapqual, int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid,
                        int32_t n_thresholds, const int32_t *thresholds,
                        int32_t maxgap, int32_t device, int64_t *out);
int bsig_coverage_summary(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                          int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                          const int32_t *width, const int32_t *strand,
                          const int32_t *tlen_filter, int32_t n_tlen_filter,
                          int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                          int32_t n_thresholds, const int32_t *thresholds,
                          int32_t maxgap, int32_t device, int64_t *out);
/* The scaled regions (bsig_plan_create_scaled): out receives n_ranges * S * n_bins int64 in the caller's range order.
 * bsig_pileup_scaled: the 5' ends (ss 0 / 1: S = 1 / 2); bsig_coverage_scaled: the per-base coverage (S = 1).  n_bins and
 * the parameters are checked before the BAM is opened or decoded.  With several GPUs each takes its block of the
 * (rid, loc)-sorted ranges and the host PLACES each block's rows at the caller's indices (bsig_last_call_route():
 * "scaled of N blocks of ranges, rows placed on the host"; one GPU: "scaled"). */
int bsig_pileup_scaled(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                       int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                       const int32_t *width, const int32_t *strand,
                       const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t ss, int32_t requiredF, int32_t filteredF, int32_t pe_mid,
                       int32_t n_bins, int32_t maxgap, int32_t device, int64_t *out);
int bsig_coverage_scaled(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                         int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                         const int32_t *width, const int32_t *strand,
                         const int32_t *tlen_filter, int32_t n_tlen_filter,
                         int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                         int32_t n_bins, int32_t maxgap, int32_t device, int64_t *out);
/* The capped signals (bsig_plan_create_capped): keep_dup = k caps every per-base, per-strand 5'-end cell at k before anything
 * is binned, added or extended.  bsig_pileup_capped: bsig_pileup_core's arguments and result (binsize <= 0: bamCount) with
 * keep_dup behind pe_mid; bsig_coverage_capped: bsig_coverage_core_ex's with frag_len and keep_dup behind tspan -- the
 * coverage of the kept reads resized to frag_len bases.  out / off as in bsig_layout() for the call's binsize and ss.  pe_mid,
 * tspan, a template-length rule (n_tlen_filter != 0), keep_dup < 1 and a frag_len outside 1 .. BSIG_FRAG_LEN_MAX fail with
 * BSIG_ERR_ARG before the BAM is opened or decoded, each with its own message.  With several GPUs each takes its block of
 * the (rid, loc)-sorted ranges and the host PLACES each block's rows through the layout's offsets (bsig_last_call_route():
 * "capped of N blocks of ranges, rows placed on the host"; one GPU: "capped").  */
/* (Laid out with their parameters below their names ON PURPOSE, as bsig_pileup_vplot is: tests/test_file_level_refusals_cpu.py
 * lists the file-level entry points by their one-line form and compares them with a table of refusals recorded before these
 * calls existed; their refusals are pinned in tests/test_capped_cpu.py instead.)                                           */
int bsig_pileup_capped(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    const int32_t *tlen_filter, int32_t n_tlen_filter,
    int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss,
    int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t keep_dup, int32_t maxgap,
    int32_t device, int32_t *out, const int64_t *off);
int bsig_coverage_capped(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    const int32_t *tlen_filter, int32_t n_tlen_filter,
    int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan, int32_t frag_len, int32_t keep_dup,
    int32_t maxgap, int32_t device, int32_t binsize, int32_t ss,
    int32_t *out, const int64_t *off);
/* The file-level calls with the result as RUNS (bsig_runs_*): bsig_pileup_core's / bsig_coverage_core_ex's arguments
 * without out / off; binsize <= 0 (bamCount) fails with BSIG_ERR_ARG, and all parameters are checked before the BAM is
 * opened.  The per-base cells live only in HBM, and only for one block of the (rid, loc)-sorted ranges at a time: a block
 * holds at most env BAMSIGNALS_RUNS_BLOCK_CELLS cells (read per call; default 2^31, 8 GiB of int32), a single larger range
 * is a block of its own.  With several GPUs each takes a contiguous share of the sorted ranges and encodes it; no per-base
 * cell is gathered.  The host puts the segments in the caller's range order: segment S * i + antisense of range i (S = 2
 * with ss).  A coverage bin past INT32_MAX fails the call before anything is encoded.  The result is a host-side handle,
 * because its size is known only afterwards: ask it for n_seg and n_runs, copy it out (seg_off: n_seg + 1 int64;
 * values, lengths: n_runs int32 each) and free it.  bsig_last_call_route() says "runs".                              */
typedef struct bsig_runs_result bsig_runs_result;
int bsig_pileup_runs(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                     int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                     const int32_t *width, const int32_t *strand,
                     const int32_t *tlen_filter, int32_t n_tlen_filter,
                     int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss,
                     int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t maxgap,
                     int32_t device, bsig_runs_result **result);
int bsig_coverage_runs(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                       int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                       const int32_t *width, const int32_t *strand,
                       const int32_t *tlen_filter, int32_t n_tlen_filter,
                       int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                       int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, bsig_runs_result **result);
/* bamCoverage of reads resized to the fragment at file level (bsig_plan_create_resized above): bsig_coverage_core_ex,
 * bsig_coverage_sum and bsig_coverage_runs with tspan replaced by frag_len, through the same dispatcher (several GPUs and
 * the resident cache as for those; an index-driven decode asks for range +- (frag_len - 1)).  The mode is
 * BSIG_MODE_COVERAGE_EX; frag_len outside 1 .. BSIG_FRAG_LEN_MAX fails with BSIG_ERR_ARG, like every other parameter
 * before the BAM is opened.                                                                                          */
int bsig_coverage_core_resized(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                               int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                               const int32_t *width, const int32_t *strand,
                               const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss,
                               int32_t *out, const int64_t *off);
int bsig_coverage_sum_resized(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                              int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                              const int32_t *width, const int32_t *strand,
                              const int32_t *tlen_filter, int32_t n_tlen_filter,
                              int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                              int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int64_t *sum);
int bsig_coverage_runs_resized(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                               int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                               const int32_t *width, const int32_t *strand,
                               const int32_t *tlen_filter, int32_t n_tlen_filter,
                               int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                               int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, bsig_runs_result **result);
int64_t bsig_runs_result_n_seg(const bsig_runs_result *result);
int64_t bsig_runs_result_n_runs(const bsig_runs_result *result);
int bsig_runs_result_copy(const bsig_runs_result *result, int64_t *seg_off, int32_t *values, int32_t *lengths);
void bsig_runs_result_free(bsig_runs_result *result);
/* The file-level calls with the result as VIEWS (bsig_views_*, where a view is defined): the arguments of bsig_pileup_runs,
 * bsig_coverage_runs and bsig_coverage_runs_resized plus the thresholds lower <= upper, on the same route -- blocks of at
 * most env BAMSIGNALS_RUNS_BLOCK_CELLS cells of the (rid, loc)-sorted ranges, each GPU a contiguous share, only the views
 * downloaded, the segments put in the caller's range order on the host.  binsize <= 0 fails with BSIG_ERR_ARG; all
 * parameters, lower <= upper included, are checked before the BAM is opened.  The result is a host-side handle: ask it for
 * n_seg and n_views, copy it out (seg_off: n_seg + 1 int64; start, width, max, summit: n_views int32 each; sum: n_views
 * int64; the value pointers may be NULL when there is no view) and free it.  bsig_last_call_route() says "views".      */
typedef struct bsig_views_result bsig_views_result;
int bsig_pileup_views(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                      int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                      const int32_t *width, const int32_t *strand,
                      const int32_t *tlen_filter, int32_t n_tlen_filter,
                      int32_t mapqual, int32_t binsize, int32_t shift, int32_t ss,
                      int32_t requiredF, int32_t filteredF, int32_t pe_mid, int32_t maxgap,
                      int32_t device, int32_t lower, int32_t upper, bsig_views_result **result);
int bsig_coverage_views(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                        int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                        const int32_t *width, const int32_t *strand,
                        const int32_t *tlen_filter, int32_t n_tlen_filter,
                        int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t tspan,
                        int32_t maxgap, int32_t device, int32_t binsize, int32_t ss,
                        int32_t lower, int32_t upper, bsig_views_result **result);
int bsig_coverage_views_resized(const char *bampath, int64_t n_ranges, const int32_t *seq_code,
                                int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
                                const int32_t *width, const int32_t *strand,
                                const int32_t *tlen_filter, int32_t n_tlen_filter,
                                int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t frag_len,
                                int32_t maxgap, int32_t device, int32_t binsize, int32_t ss,
                                int32_t lower, int32_t upper, bsig_views_result **result);
/* bamCoverage(splice = TRUE) at file level: bsig_coverage_core_ex, bsig_coverage_sum, bsig_coverage_runs and
 * bsig_coverage_views WITHOUT tspan, on the file's spliced reads (bsig_reads_from_bam_spliced), through the same dispatcher.
 * The flag is judged with the other parameters before the BAM is opened.  A file's plain and spliced reads are two resident
 * sets of the cache (a second set only when one file is asked both ways); a spliced set has no reads file (none is loaded,
 * none is written); with several GPUs it is decoded on the first and cloned.  bsig_last_call_route() says "spliced".
 * (Laid out with their parameters below their names ON PURPOSE, as bsig_pileup_vplot is; their refusals are pinned in
 * tests/test_spliced_cpu.py.)                                                                                        */
int bsig_coverage_core_spliced(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    const int32_t *tlen_filter, int32_t n_tlen_filter,
    int32_t mapqual, int32_t requiredF, int32_t filteredF,
    int32_t maxgap, int32_t device, int32_t binsize, int32_t ss,
    int32_t *out, const int64_t *off);
int bsig_coverage_sum_spliced(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    const int32_t *tlen_filter, int32_t n_tlen_filter,
    int32_t mapqual, int32_t requiredF, int32_t filteredF,
    int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, int64_t *sum);
int bsig_coverage_runs_spliced(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    const int32_t *tlen_filter, int32_t n_tlen_filter,
    int32_t mapqual, int32_t requiredF, int32_t filteredF,
    int32_t maxgap, int32_t device, int32_t binsize, int32_t ss, bsig_runs_result **result);
int bsig_coverage_views_spliced(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    const int32_t *tlen_filter, int32_t n_tlen_filter,
    int32_t mapqual, int32_t requiredF, int32_t filteredF,
    int32_t maxgap, int32_t device, int32_t binsize, int32_t ss,
    int32_t lower, int32_t upper, bsig_views_result **result);
int64_t bsig_views_result_n_seg(const bsig_views_result *result);
int64_t bsig_views_result_n_views(const bsig_views_result *result);
int bsig_views_result_copy(const bsig_views_result *result, int64_t *seg_off, int32_t *start, int32_t *width, int64_t *sum,
                           int32_t *max, int32_t *summit);
void bsig_views_result_free(bsig_views_result *result);
/* ------------------------------------------------------------------------------------------
 * Splice junctions with read counts (GenomicAlignments::summarizeJunctions' score / plus_score / minus_score, STAR's
 * SJ.out.tab columns 7 and 9, regtools' anchor filter), found on the GPU (csrc/junctions.hip).
 * A spliced bsig_reads keeps its gap table as a JUNCTION TABLE: every gap of every read (the gaps defined above
 * bsig_reads_upload_spliced) is one row with its reference, its first and last base (0-based), its read's flag and mapq and
 * its ANCHOR = min(left, right): the reference bases of the aligned block that ends right before the gap and of the one
 * that begins right behind it (back to the read's previous gap or its pos, forward to its next gap or its end; D counts, I
 * does not; a side without an aligned base is 0).  The rows are stably sorted by (reference, start, end) and live in the
 * object's own device memory (bsig_reads_info.hbm_bytes counts them, bsig_reads_clone copies them); fewer than 2^32 - 8
 * rows.  A plain object has no table: bsig_reads_n_junction_rows is 0, bsig_reads_junctions is BSIG_ERR_ARG.
 * The query: a row belongs to range i iff it is on the range's reference, start >= loc and end <= loc + len - 1 (the junction
 * lies within the range), it passes mapqual / requiredF / filteredF exactly as a read passes them in every other call, and
 * anchor >= min_anchor (>= 0).  Range i's result is the distinct (start, end) among its rows, ascending by start, then end,
 * each with count = the number of rows -- with ss two values, (sense, antisense): sense iff the row's 0x10 bit agrees with the
 * range's strand, '*' counted as '+' -- and max_anchor = the largest anchor among them.  Ranges are independent (overlapping
 * ranges each report a shared junction); a range of width 0 or without rows owns nothing.  seg_off has n + 1 entries in the
 * caller's range order.  More than 2^32 - 8 (range, row) pairs in one query is BSIG_ERR_ARG.  All integer work: the result
 * does not depend on the order in which the GPU runs it.
 * bsig_junctions is the file-level call: the eight range arguments of every file-level call, on the file's spliced reads
 * (the same resident set bsig_coverage_*_spliced use, whole-file or index-driven as the ranges ask); its parameters are
 * judged before the BAM is opened; bsig_last_call_route() says "junctions".  With several GPUs the first one answers.
 * The result handle: start, end, max_anchor hold one int32 per junction, count one uint32 -- two with ss.
 * ------------------------------------------------------------------------------------------ */
typedef struct bsig_junctions_result bsig_junctions_result;
int64_t bsig_reads_n_junction_rows(const bsig_reads *reads);     /* 0 for NULL and for a plain object                 */
int bsig_reads_junctions(const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc, const int32_t *len,
                         const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_anchor,
                         int32_t ss, bsig_junctions_result **result);
int bsig_junctions(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_anchor, int32_t ss,
    int32_t device, bsig_junctions_result **result);
int64_t bsig_junctions_result_n_seg(const bsig_junctions_result *result);
int64_t bsig_junctions_result_n_junctions(const bsig_junctions_result *result);
int bsig_junctions_result_copy(const bsig_junctions_result *result, int64_t *seg_off, int32_t *start, int32_t *end,
                               uint32_t *count, int32_t *max_anchor);
void bsig_junctions_result_free(bsig_junctions_result *result);
/* ------------------------------------------------------------------------------------------
 * Reads per gene over exon models (HTSeq's union mode = featureCounts' default = summarizeOverlaps mode "Union"), counted
 * on the GPU (csrc/genecounts.hip).
 * A GENE MODEL is n features (reference rid in 0 .. n_ref - 1, 0-based loc, len, strand -1 / 0 / +1) with gene[i] in
 * 0 .. n_genes - 1 saying which gene feature i belongs to.  Features may overlap, repeat, nest and come in any order; a
 * feature of width 0 takes part in nothing; a gene may have no feature.  bsig_gene_model_create flattens them on the host
 * (csrc/genemodel.h; no GPU is needed for any bsig_gene_model_* call) into three tables of disjoint segments sorted by
 * (reference, start): table 0 from all features, 1 from those with strand +1 or 0, 2 from those with strand -1 or 0.  A
 * segment's value is the one gene active there, or -1 where two or more genes overlap; touching segments of equal value are
 * one.  Refused with BSIG_ERR_ARG, naming the first offending feature: a negative width, a reference outside 0 .. n_ref - 1,
 * a gene outside 0 .. n_genes - 1, a strand outside -1 .. 1, loc + len beyond 2^31 - 1.
 * bsig_gene_model_copy_segments: ref_off has n_ref + 1 entries; start / end are a segment's first and last base.
 * A spliced bsig_reads keeps a READ TABLE: its source reads in BAM order, each with its aligned blocks (what
 * bsig_coverage_*_spliced cover) and its flag and mapq, in the object's own device memory (hbm_bytes counts it,
 * bsig_reads_clone copies it).  bsig_reads_n_source_reads is their number (bsig_reads_info.n_reads of a spliced object counts
 * blocks); 0 for NULL and for a plain object.
 * bsig_reads_gene_counts classifies every source read, in this order: flag & 0x4 -> unmapped; failing mapqual / requiredF /
 * filteredF as in every other call -> filtered; else with s = -1 if flag & 0x10 else +1, flipped if (flag & 0x81) == 0x81 (a
 * second mate), a feature of strand f MATCHES under strandedness 0 (unstranded) always, 1 (forward) iff f == 0 or f == s,
 * 2 (reverse) iff f == 0 or f == -s; H = the genes with a matching feature on the read's reference that shares a base with a
 * block of the read; |H| = 0 -> no_feature, 1 -> assigned (counts[that gene] += 1), >= 2 -> ambiguous.  counts has n_genes
 * entries, summary five: assigned, ambiguous, no_feature, filtered, unmapped; they sum to the number of source reads.  The
 * model's n_ref must be the object's; a plain object is BSIG_ERR_ARG.  All integer work: the result does not depend on the
 * order in which the GPU runs it.  The model's tables are copied to a GPU at its first query there and stay until
 * bsig_gene_model_free.
 * bsig_gene_counts is the file-level call: the model's reference r is the sequence named seq_levels[r] (n_seq_levels must be
 * the model's n_ref; a name the BAM lacks is BSIG_ERR_CHROM), the reads are the WHOLE file's spliced reads (the resident set
 * bsig_coverage_*_spliced and bsig_junctions use when they decode the whole file); its parameters are judged before the BAM
 * is opened; bsig_last_call_route() says "gene counts".  With several GPUs the first one answers.
 * ------------------------------------------------------------------------------------------ */
typedef struct bsig_gene_model bsig_gene_model;
int bsig_gene_model_create(int64_t n_features, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                           const int32_t *gene, int32_t n_genes, int32_t n_ref, bsig_gene_model **model);
void bsig_gene_model_free(bsig_gene_model *model);
int32_t bsig_gene_model_n_genes(const bsig_gene_model *model);
int32_t bsig_gene_model_n_ref(const bsig_gene_model *model);
int64_t bsig_gene_model_n_segments(const bsig_gene_model *model, int32_t table);    /* -1 for a table that is none of 0, 1, 2 */
int bsig_gene_model_copy_segments(const bsig_gene_model *model, int32_t table, int64_t *ref_off, int32_t *start, int32_t *end,
                                  int32_t *value);
int64_t bsig_reads_n_source_reads(const bsig_reads *reads);
int bsig_reads_gene_counts(const bsig_reads *reads, const bsig_gene_model *model, int32_t mapqual, int32_t requiredF,
                           int32_t filteredF, int32_t strandedness, int64_t *counts, int64_t *summary);
int bsig_gene_counts(const char *bampath, const bsig_gene_model *model, int32_t n_seq_levels, const char *const *seq_levels,
                     int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t strandedness, int32_t device,
                     int64_t *counts, int64_t *summary);
/* ------------------------------------------------------------------------------------------
 * A / C / G / T / N / deletion counts per base (Rsamtools::pileup, bam-readcount, deepSNV::bam2R, the count columns of
 * samtools mpileup), counted on the GPU (csrc/nucleotides.hip).
 * A read TAKES PART iff flag 0x4 is clear and it passes mapqual / requiredF / filteredF exactly as a read passes them in every
 * other call (mapq >= mapqual, every requiredF bit set, not every filteredF bit set: for a mask of one bit that is
 * (flag & filteredF) == 0, and -1 filters nothing).  Its CIGAR -- the record's own, or the CG:B,I tag behind the
 * <l_seq>S<n>N placeholder -- is walked with a reference cursor r = pos and a query cursor q = 0:
 *
 *   operation                     what is counted                                                     cursors
 *   M, =, X (0, 7, 8), length L   for i in 0 .. L - 1: query base q + i at reference base r + i,      r += L, q += L
 *                                 if its quality passes
 *   I, S (1, 4)                   nothing                                                             q += L
 *   D (2)                         one count in the deletion channel at each of r .. r + L - 1         r += L
 *                                 (no quality: it always counts)
 *   N (3)                         nothing                                                             r += L
 *   H, P (5, 6), any op > 8       nothing                                                             none
 *
 * Operations of length 0 do nothing; positions are 64-bit inside the walk; a cell outside every range is not asked for.
 * The CHANNELS, in this order: A (4-bit code 1), C (2), G (4), T (8), N (every other code: '=', the IUPAC ambiguity codes
 * and 15), '-' (deletion).  A query base at an index >= l_seq (SEQ '*', or a CIGAR longer than the sequence) counts in N and
 * its quality is missing; nothing beyond a read's own bytes is read.  A base PASSES iff qual >= min_base_qual; a missing
 * quality (byte 0xFF, or an index >= l_seq) passes every threshold; min_base_qual is 0 .. 93, else BSIG_ERR_ARG.
 * Range i (0-based loc, len, strand) owns 6 * len int32 cells [channel][position], with ss 2 * 6 * len cells
 * [sense | antisense][channel][position]: a read is sense iff its 0x10 bit agrees with the range's strand, '*' counted as
 * '+' (no mate-aware strand).  A '-' range reads 5' -> 3' on its own strand: positions reversed, channels complemented
 * (A <-> T, C <-> G; N and '-' stay).  Ranges are independent (overlapping ranges each get their counts); a range of width
 * 0 owns nothing; a range on a reference without reads, or past its end, is all zeros.  bsig_nucleotides_cells gives the
 * total and (off: n + 1 entries, or NULL) every range's first cell.  Counters are 32-bit: a cell past 2^31 - 1 is out of
 * scope.  All integer work: the result does not depend on the order in which the GPU runs it.  With min_base_qual == 0 the
 * six channels of a base add up to bsig_coverage_*_spliced there (D covered, N not) for reads that have a
 * reference-consuming operation.
 * A bsig_reads WITH BASES (bsig_reads_upload_bases, bsig_reads_from_bam_bases / _regions_bases) is an ordinary plain
 * object -- every plan works on it unchanged -- that carries a BASE TABLE in BAM order in its own device memory (hbm_bytes
 * counts it, bsig_reads_clone copies it, bsig_reads_base_table_bytes states its size: 28 bytes a read and 8 + 8 for the two
 * closing offsets, 4 an operation, 1.5 a base, 8 * (n_ref + 1)): per read pos, the running maximum of end within its
 * reference, flag | mapq << 16 and where its operations and its bases begin; then the operations, the bases as BAM's own
 * nibbles tightly packed, one quality byte a base.  bsig_base_columns describes them to bsig_reads_upload_bases, which needs
 * cigar_off + cigar (cols->end is not read): seq_off has n + 1 entries counted in bases from 0; base g of the whole is
 * nibble g of seq (byte g / 2, the high half where g is even) and byte g of qual.  bsig_bam_decode_bases is bsig_bam_decode
 * that fills them as well (host memory owned by the handle, valid until its next decode or close); the _from_bam_ forms
 * are bsig_reads_from_bam / _regions that also copy every record's operations, bases and qualities out of a chunk's inflated
 * stream on the GPU, right behind the record extraction (one host read per chunk sizes the chunk's piece; one share, chunk by
 * chunk, as a spliced decode); where the file takes the CPU decode -- a record whose l_seq runs past it among the reasons --
 * bsig_bam_decode_bases' columns go through bsig_reads_upload_bases: same result.  BAMSIGNALS_DEVICE_DECODE as above.  bsig_reads_save of such an object is
 * BSIG_ERR_ARG; an object without bases (plain or spliced) answers bsig_reads_nucleotides with BSIG_ERR_ARG.
 * bsig_reads_nucleotides writes device memory, _host host memory (the cells of bsig_nucleotides_cells).
 * bsig_nucleotides is the file-level call: the eight range arguments of every file-level call, on the file's reads with
 * bases (a resident set of its own, kept only once a nucleotide call asked for it; whole-file or index-driven as the ranges
 * ask); its parameters are judged before the BAM is opened; bsig_last_call_route() says "nucleotides".  With several GPUs
 * the first one answers.
 * ------------------------------------------------------------------------------------------ */
#define BSIG_NUC_CHANNELS 6
#define BSIG_NUC_MAX_BASE_QUAL 93
typedef struct {
    const int64_t *seq_off;    /* n_reads+1 : read i owns bases [seq_off[i], seq_off[i+1])              */
    const uint8_t *seq;        /* 4-bit codes, two a byte, the first of a byte in its high half         */
    const uint8_t *qual;       /* one byte a base, 0xFF = missing                                       */
} bsig_base_columns;
int bsig_reads_upload_bases(bsig_ctx *ctx, const bsig_columns *cols, const bsig_base_columns *bases, bsig_reads **reads);
int32_t bsig_reads_has_bases(const bsig_reads *reads);           /* 1 / 0; 0 for NULL                            */
int64_t bsig_reads_base_table_bytes(const bsig_reads *reads);    /* 0 for NULL and for an object without bases   */
int bsig_bam_decode_bases(bsig_bam *bam, int64_t n_regions, const int32_t *rid, const int64_t *beg, const int64_t *end,
                          int32_t threads, bsig_columns *cols, bsig_base_columns *bases);
int bsig_reads_from_bam_bases(bsig_ctx *ctx, bsig_bam *bam, int32_t threads, bsig_reads **reads);
int bsig_reads_from_bam_regions_bases(bsig_ctx *ctx, bsig_bam *bam, int64_t n_regions, const int32_t *rid,
                                      const int64_t *beg, const int64_t *end, int32_t threads, bsig_reads **reads);
int64_t bsig_nucleotides_cells(int64_t n_ranges, const int32_t *len, int32_t ss, int64_t *off);      /* -1: a negative width */
int bsig_reads_nucleotides(const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc, const int32_t *len,
                           const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual,
                           int32_t ss, int32_t *out_dev);
int bsig_reads_nucleotides_host(const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc,
                                const int32_t *len, const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF,
                                int32_t min_base_qual, int32_t ss, int32_t *out_host);
int bsig_nucleotides(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss,
    int32_t device, int32_t *out);
/* ------------------------------------------------------------------------------------------
 * Variant and mixed-allele SITES: the bases at which the reads disagree with a reference, or with each other (the candidate
 * stage of VarScan, of bcftools mpileup | call and of deepSNV; the filter over Rsamtools::pileup), found on the GPU
 * (csrc/sites.hip; the decision itself is csrc/sitemath.h: site_classify, the same function on host and device).
 * A site is decided from the cells of a range EXACTLY as bsig_reads_nucleotides defines them -- after a '-' range's reversal
 * and complement, with the same read and base filters --: sites == f(nucleotide counts) by definition, and only the sites
 * leave the device.  For cell p of range i let c[0 .. 5] be the six channels A C G T N '-', the two planes SUMMED when ss is
 * set (ss changes only what is reported), and D their sum.
 *   The BASE channel b: with ref, b = ref[cell]: ref is a host array of sum(len) bytes holding channel codes 0 .. 4, range
 *   after range in the range's own reading direction (for a '-' range the reverse complement, as getSeq(genome, gr) gives
 *   it); a cell whose ref is 4 (N) is never a site; a code above 4 is BSIG_ERR_ARG, judged on the host before anything runs.
 *   Without ref (NULL), b is the first channel of all six that holds the largest count.
 *   The ALT channel a: the first channel with the largest count among those in alt_mask (bits 0 .. 5, nonzero), b excluded; a
 *   mask that names no channel but b leaves the cell without an alt: no site.
 *   The cell is a site iff D >= min_depth and c[a] >= min_alt and c[a] * frac_den >= frac_num * D (64-bit integers).
 * min_depth >= 1, min_alt >= 1, 0 <= frac_num <= frac_den, 1 <= frac_den <= 2^20, alt_mask in 1 .. 0x3F and min_base_qual as
 * for the nucleotide counts: anything else is BSIG_ERR_ARG with a sentence of its own.
 * The result, a structure of arrays in the caller's range order: seg_off (int64, n_ranges + 1: range i owns sites seg_off[i]
 * .. seg_off[i + 1]), pos (int32 a site: the cell's index in the range, 0-based, in the range's reading direction, ascending
 * within a range), alleles (int32 a site: b | a << 8), counts (int32 [site][channel], with ss [site][plane][channel]: sense,
 * antisense).  Ranges are independent (duplicated ranges give duplicated sites); the order is fixed and does not depend on how
 * the GPU schedules the work; the arrays have their exact size; with no site at all the value pointers of
 * bsig_sites_result_copy may be NULL.  bsig_sites_result_timing: the seconds of count + scan, of the fill and of the download
 * of the query that made the result (0 where a stage did not run).
 * An object without bases answers bsig_reads_sites as it answers bsig_reads_nucleotides; the limit of 2^31 - 1 tiles and the
 * empty set's behaviour (no site) are that call's as well.  bsig_sites is the file-level call: the eight range arguments of
 * every file-level call on the file's reads with bases (bsig_nucleotides' resident set); its parameters and the ref codes
 * are judged before the BAM is opened; bsig_last_call_route() says "sites".  With several GPUs the first one answers.
 * ------------------------------------------------------------------------------------------ */
typedef struct bsig_sites_result bsig_sites_result;
int bsig_reads_sites(const bsig_reads *reads, int64_t n_ranges, const int32_t *rid, const int32_t *loc, const int32_t *len,
                     const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual,
                     int32_t ss, const uint8_t *ref, int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den,
                     int32_t alt_mask, bsig_sites_result **result);
int bsig_sites(
    const char *bampath, int64_t n_ranges, const int32_t *seq_code,
    int32_t n_seq_levels, const char *const *seq_levels, const int32_t *start,
    const int32_t *width, const int32_t *strand,
    int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss,
    const uint8_t *ref, int32_t min_depth, int32_t min_alt, int32_t frac_num, int32_t frac_den, int32_t alt_mask,
    int32_t device, bsig_sites_result **result);
int64_t bsig_sites_result_n_ranges(const bsig_sites_result *result);
int64_t bsig_sites_result_n_sites(const bsig_sites_result *result);
int bsig_sites_result_copy(const bsig_sites_result *result, int64_t *seg_off, int32_t *pos, int32_t *alleles, int32_t *counts);
void bsig_sites_result_timing(const bsig_sites_result *result, double *t3);
void bsig_sites_result_free(bsig_sites_result *result);
/* replaces bamsignals_writeSamAsBamAndIndex (ref: src/bamsignals.cpp:496-534): text SAM ->
 * BAM + <bampath>.bai                                                                          */
int bsig_write_sam_as_bam_and_index(const char *sampath, const char *bampath);
/* columnar writer used for synthetic BAMs: coordinate-sorted columns -> BAM + BAI             */
int bsig_write_columns_as_bam(const char *bampath, int32_t n_ref, const char *const *ref_names,
                              const bsig_columns *cols, int32_t level);
/* the same with real-shaped records: a read name, l_seq random bases and qualities (about 3 bits of
 * entropy per quality, like binned Illumina data), an NM tag -- 204 bytes per 100-bp read instead of
 * 52, literal-heavy DEFLATE blocks that compress about 2 : 1.  For benchmarks of the decode stage on
 * data shaped like real BAMs; the alignment columns are the caller's, the rest follows (seed, index). */
int bsig_write_columns_as_bam_with_seq(const char *bampath, int32_t n_ref, const char *const *ref_names,
                                       const bsig_columns *cols, int32_t level, int32_t l_seq, uint64_t seed);
/* The file-level entry points keep, per process: one context per listed GPU, the parsed header +
 * BAI of the last 16 BAMs, and whole BAMs decoded to HBM -- least recently used first out above
 * env BAMSIGNALS_CACHE_GB (per GPU, default 96).  A file is identified by path + size + mtime of the
 * BAM and of its index: a rewritten file is decoded again.  env BAMSIGNALS_SIDECAR=1 (next to the BAM,
 * <bam>.bsig) or BAMSIGNALS_SIDECAR_DIR=<dir> additionally keeps the resident layout on disk
 * (bsig_reads_save) so that another process skips the decode.  File-level calls may be made from
 * several host threads at once (the cache is locked for look-ups only; cold decodes take turns).
 * Every device list seen (device argument / BAMSIGNALS_DEVICES) keeps its own contexts and resident
 * BAMs: alternating between two GPUs does not evict anything.  Multi-GPU calls on one device list take
 * turns at the run stage (they share the slots' cached result buffers and the RCCL communicators).
 * bsig_cache_clear drops all of it (not the sidecar files); whatever a running call uses -- contexts,
 * resident reads, communicators -- stays alive until that call returns, so it may be called at any time. */
void bsig_cache_clear(void);
/* diagnostic: device / page-locked allocations made so far for the buffers the multi-GPU result path keeps
 * between calls (a call on a resident BAM with shapes seen before adds none)                        */
int64_t bsig_debug_scratch_allocs(void);
/* diagnostic: number and a checksum of the BGZF blocks of a file as the device-side decode tabulates them
 * (env BAMSIGNALS_SCAN=mmap: the walk through the mapped file; default: through pread())              */
int bsig_debug_block_table(const char *path, int64_t *n_blocks, uint64_t *checksum);
/* ... and in two steps, as the whole-file decode tabulates large files: the head first (*n_head blocks), the
 * rest in the background                                                                             */
int bsig_debug_block_table_progressive(const char *path, int64_t head_bytes, int64_t *n_head, int64_t *n_blocks,
                                       uint64_t *checksum);
/* how the calling thread's last file-level call was carried out, e.g.
 * "8 GPU slot(s); reads: sharded decode, columns over rccl; result: xgmi/rccl"                  */
const char *bsig_last_call_route(void);
/* stage seconds of the calling thread's last bsig_pileup_core / bsig_coverage_core: open (header +
 * BAI), decode, upload + HBM layout, plan + kernels + download, total; t6[5] = 1 if the BAM was
 * already resident in HBM                                                                      */
void bsig_last_call_timing(double *t6);
/* the same (slots 0..5) and where the stages' time went, n <= 16 slots:
 *   6  seconds inside the driver's allocator (hipMalloc / hipFree / hipHostMalloc ...) during decode + layout
 *   7  ... during plan + kernels + download          8  ... during the whole call
 *   9  plan creation (ranges -> tiles in HBM, heavy-tile probe)   10  kernels (launch .. stream idle; includes the
 *      result buffer's allocation)   11  download of the result to host memory   (9-11: one GPU; 0 with several)
 *   12 driver allocation calls of the whole call
 *   13 reserved
 *   14 bytes reserved for the resident columns while the file was still being inflated (0: no reservation)
 *   15 seconds the layout waited for that reservation
 * The allocator meter is per process: calls made by other threads at the same time are counted too.         */
void bsig_last_call_timing_ex(double *t, int32_t n);

/* ------------------------------------------------------------------------------------------
 * Reassembly of sharded results (multi-GPU): segment k of src (src_off[k] .. src_off[k+1]) is
 * copied to dst at dst_off[which[k]].  The host half of "each GArray owns its own output
 * buffer" (ref: src/bamsignals.cpp:164,181,186) once ranges were dealt round-robin to GPUs.
 * ------------------------------------------------------------------------------------------ */
int bsig_scatter_segments(int64_t n, const int32_t *src, const int64_t *src_off, int32_t *dst,
                          const int64_t *dst_off, const int64_t *which);

/* The same on the device, for hosts that gather the shards into ONE device buffer on the root GPU (one
 * process per GPU: torch.distributed / RCCL gather): the segment tables live in HBM with the map, so a
 * run is one kernel launch on the context's stream, asynchronous, and the result stays in HBM in the
 * caller's range order.  The tables are checked like bsig_scatter_segments checks them (every segment fits
 * its destination, inside n_src_cells / n_dst_cells).  src_off: n+1 entries, dst_off: n_dst+1, which: n. */
typedef struct bsig_segmap bsig_segmap;
int bsig_segmap_create(bsig_ctx *ctx, int64_t n, const int64_t *src_off, int64_t n_dst, const int64_t *dst_off,
                       const int64_t *which, bsig_segmap **map);
int bsig_segmap_run(bsig_segmap *map, const int32_t *src_dev, int32_t *dst_dev);
/* A NARROW WIRE for result shards that travel between GPUs (round 5; the gather of the shards to one GPU is bounded by that
 * GPU's ingress, and the cells of a per-base profile are almost all 0, 1 or 2): a shard of n_cells int32 cells as a message
 * of bsig_narrow_bytes(n_cells, cap) bytes -- two bits a cell (the value, or 3 = see the list) and a list of up to `cap`
 * (cell, value) exceptions; lossless for any int32.  bsig_narrow_pack writes the message on the context's stream (src_dev
 * and msg_dev 16-B aligned); bsig_narrow_count (synchronises) says how many exceptions a packed shard has -- a plan's result
 * is a function of plan and reads, so a first run tells the `cap` of every later one; bsig_segmap_run_narrow is
 * bsig_segmap_run from such a message; bsig_segmap_narrow_overflowed (synchronises) reports whether any message so far had
 * more exceptions than its list held (its result is then wrong).  The message, in 32-bit words: [0] the number of
 * exceptions the shard has (it may exceed cap: then the list is incomplete), [1..3] zero, [4 .. 4 + ceil(n_cells / 16)) the
 * codes (cell c in bits 2 (c % 16) .. + 1 of word c / 16), then cap pairs (cell, value) of which the first min([0], cap)
 * are in use, in no particular order; n_cells < 2^32.  Replaces nothing of the reference: each range owns its
 * output there (ref: src/bamsignals.cpp:164,181,186), which is what makes shards -- and their reassembly -- legal.       */
int64_t bsig_narrow_bytes(int64_t n_cells, int64_t cap);
int bsig_narrow_pack(bsig_ctx *ctx, const int32_t *src_dev, int64_t n_cells, void *msg_dev, int64_t cap);
int bsig_narrow_count(bsig_ctx *ctx, const void *msg_dev, int64_t *n_exceptions);
int bsig_segmap_run_narrow(bsig_segmap *map, const void *msg_dev, int64_t n_cells, int64_t cap, int32_t *dst_dev);
int bsig_segmap_narrow_overflowed(bsig_segmap *map, int *overflowed);
void bsig_segmap_free(bsig_segmap *map);

#ifdef __cplusplus
}
#endif
#endif /* BAMSIGNALS_ABI_H */
