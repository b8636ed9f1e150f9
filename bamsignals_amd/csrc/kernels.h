// Launchers of the gfx950 kernels (kernels.hip), used by the host runtime (runtime.hip).
#ifndef BSIG_KERNELS_H
#define BSIG_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bamsignals_abi.h"
#include "bsig_types.h"

// k_summary_tiles' thresholds, a kernel argument: t[0 .. k) rising, the rest 2^32 - 1
struct BsigThresholds {
    uint32_t t[BSIG_SUMMARY_MAX_THRESHOLDS];
    int32_t k;
};

namespace bsig {

struct ScatterPtrs {
    int32_t *pos[BSIG_MAX_CLASSES];
    int32_t *end[BSIG_MAX_CLASSES];
    uint32_t *fm[BSIG_MAX_CLASSES];
    int32_t *tlen[BSIG_MAX_CLASSES];
    uint32_t *gb[BSIG_MAX_CLASSES];
    int32_t kshift[BSIG_MAX_CLASSES];
};

hipError_t launch_pileup(int mode, int ss, int threads, const BsigReadsDev &R, const BsigKParams &P,
                         const BsigWorkItem *items, int64_t n_items, int tile_cells,
                         void *windows /* n_items * BSIG_MAX_CLASSES * 8 bytes (fixed read ranges: slices of heavy tiles), or NULL */,
                         bool resolve_first /* fill `windows` with k_resolve before the pileup launch */,
                         int32_t *out, hipStream_t st);
// the packed class's 16-bit 5'-end column (bsig_types.h: p5h) from its n words fm and the pair table fmtab: cap
// (a multiple of 8, >= n + 8) entries at `out`, those from n on zero
hipError_t launch_make_p5h(const uint32_t *fm, const uint32_t *fmtab, int64_t n, int64_t cap, uint16_t *out, hipStream_t st);
// ... and span class 0's or 1's, from its pos and fm columns (span - 1 = fm >> span_shift) and its index of n_buckets
// buckets; *bad is set to 1 if a read lies outside its reference (device arrays of n_ref entries), where the column
// must not be used
hipError_t launch_make_short_p5h(const int32_t *pos, const uint32_t *fm, int span_shift, int64_t n, int64_t cap, const uint32_t *idx,
                                 uint64_t n_buckets, int kshift, const uint32_t *ref_unit0, const uint32_t *ref_units, int n_ref,
                                 uint16_t *out, int *bad, hipStream_t st);
// the packed class's filter table for P (BSIG_PACK_CODES bytes at `out`): once per plan
hipError_t launch_make_ptab(const BsigReadsDev &R, const BsigKParams &P, uint8_t *out, hipStream_t st);
hipError_t launch_resolve(const BsigReadsDev &R, const BsigKParams &P, int mode, const BsigWorkItem *items,
                          int64_t n_items, void *windows, hipStream_t st);
hipError_t launch_count_heavy(const void *windows, int64_t n_items, int64_t heavy_reads,
                              unsigned long long *count, hipStream_t st);
hipError_t launch_cigar_end(int64_t n, const int32_t *pos, const uint16_t *flag, const int64_t *cigar_off,
                            const uint32_t *cigar, int32_t *end_out, hipStream_t st);
int64_t prep_chunks(int64_t n);
// the (flag, mapq) pairs of a sample of the short reads: hist = 2^20 zeroed counters (flag | mapq << 12), the non-empty
// ones as (key, count) in pairs[0 .. min(*n_pairs, cap))
hipError_t launch_pair_sample(int64_t n, const int32_t *pos, const int32_t *end, const uint16_t *flag, const uint8_t *mapq,
                              uint32_t *hist, uint2 *pairs, uint32_t cap, uint32_t *n_pairs, hipStream_t st);
// codemap (2^20 x uint16, filled with 0xFFFF) receives the code of every pair of fmtab (flag | mapq << 16)
hipError_t launch_codemap_fill(const uint32_t *fmtab, int n_codes, uint16_t *codemap, hipStream_t st);
hipError_t launch_span_hist(int64_t n, int32_t n_ref, const int64_t *ref_off, const uint32_t *ref_units, const int32_t *pos,
                            const int32_t *end, const uint16_t *flag, const uint8_t *mapq, const uint16_t *codemap /* or NULL */,
                            uint32_t *chunk_counts,
                            int32_t *maxspan /* BSIG_MAX_CLASSES + 1: the last = "not sorted" flag */, hipStream_t st);
// exclusive scan of the chunks' class counts (BSIG_MAX_CLASSES per chunk) and the class totals, on the device
hipError_t launch_chunk_scan(int64_t n_chunks, const uint32_t *counts, uint64_t *chunk_base, uint64_t *totals, hipStream_t st);
hipError_t launch_scatter(int64_t n, int32_t n_ref, const int64_t *ref_off, const uint32_t *ref_unit0,
                          const uint32_t *ref_units, const int32_t *pos, const int32_t *end,
                          const uint16_t *flag, const uint8_t *mapq, const int32_t *tlen, const uint16_t *codemap,
                          const uint64_t *chunk_base, const ScatterPtrs &S, hipStream_t st);
hipError_t launch_build_idx(int64_t n, const uint32_t *gb, uint64_t n_buckets, uint32_t *idx, hipStream_t st);
// 64-bit order-independent checksum of n_words 32-bit words, ADDED into *acc (device)
hipError_t launch_checksum(const void *words, uint64_t n_words, uint64_t salt, unsigned long long *acc, hipStream_t st);
// *bad (device) = 1 unless idx[0..n_buckets] is non-decreasing, <= n_reads, and ends at n_reads
hipError_t launch_check_idx(const uint32_t *idx, uint64_t n_buckets, uint32_t n_reads, int *bad, hipStream_t st);
// One instantiation of a reduction's tile kernel, as its launch and the occupancy query of the same form need it: the kernel
// (NULL: the kind has no such form), its name in the launch log, workgroup size, LDS bytes and k_resolve_tiles' mode.  A
// kind's *_form maps run-time choices to one; its launch_*_tiles picks a launch's from P (half: !wide && P.packed_half).
struct TileForm { const void *kernel; const char *name; int threads; size_t lds; int mode; };
int tile_blocks_per_cu(const TileForm &f);      // workgroups a CU holds at a time (1 if the runtime cannot say); logs nothing
// Sums over ranges of one width (bsig_plan_create_sum).  kind: 0 bamProfile, 1 coverage, 2 strand-split coverage.
// k_sum_tiles: run r = tiles [runs[r].x, runs[r].y) of one c0 -> slab r (the form's lds / 4 int32 rounded: the caller
// sizes it as tile_cells * S rounded up to 4); windows / resolve_first as in launch_pileup (P.resolved: BsigResolved
// per tile), or the fixed windows of heavy slices.  res / frag: P.resolved / P.frag_len of the launch.
TileForm sum_form(int kind, int ss, int nw, bool half, bool res, bool frag, int tile_cells);
hipError_t launch_sum_tiles(int kind, int ss, int nw, const BsigReadsDev &R, const BsigKParams &P, const BsigWorkItem *items,
                            int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows, bool resolve_first, int32_t *slab,
                            hipStream_t st);
// slabs -> per-base int64 sums (added: zero `base` first); signed for coverage differences
hipError_t launch_sum_reduce(bool is_signed, const int32_t *slab, int32_t slab_vals, const BsigSumChunk *chunks, int64_t n_chunks,
                             int32_t max_nvals, unsigned long long *base, hipStream_t st);
// coverage: prefix sums of the per-base differences that restart at every tile boundary, in place
hipError_t launch_sum_scan(long long *base, int32_t width, int32_t tile_cells, int32_t S, hipStream_t st);
// per-base sums -> n_out = n_bins * S bins (2 * bin + s)
hipError_t launch_sum_bins(const long long *base, int32_t width, int32_t binsize, int32_t S, int64_t n_out, long long *out, hipStream_t st);
// Strand cross-correlation over ranges (bsig_plan_create_xcorr).  k_xcorr_tiles: run r = tiles [runs[r].x, runs[r].y), a
// tile = item.out_off body cells (<= body) + an antisense halo, item.nc <= P.tile_cells (>= body + max_lag) cells in all;
// every workgroup ADDS its partial sums into out (max_lag + 1 lags, then the five moments; the first workgroup adds
// n_cells, the plan's count of cells, to the first moment): zero `out` first.  wide: 32-bit image cells for tiles with
// more reads than a 16-bit cell may see.  windows / resolve_first as in launch_sum_tiles (no fixed windows).
TileForm xcorr_form(int threads, bool half, bool wide, int tile_cells, int body, int max_lag);
hipError_t launch_xcorr_tiles(int threads, bool wide, const BsigReadsDev &R, const BsigKParams &P, const BsigWorkItem *items,
                              int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows, bool resolve_first, int body,
                              int max_lag, unsigned long long n_cells, unsigned long long *out, hipStream_t st);
// Fragment-length histogram over ranges (bsig_plan_create_frag).  k_frag_tiles: run r = count tiles [runs[r].x, runs[r].y);
// every workgroup ADDS its non-zero rows into out (n_rows int64): zero `out` first.  P.div_magic / P.div_shift divide by
// lenbin (>= 2).  merge: equal rows of a wave are merged before the LDS atomic.  windows / resolve_first as in
// launch_sum_tiles (no fixed windows).
TileForm frag_form(int threads, bool merge, int n_rows);
hipError_t launch_frag_tiles(int threads, bool merge, const BsigReadsDev &R, const BsigKParams &P, const BsigWorkItem *items,
                             int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows, bool resolve_first, int n_rows,
                             int lenbin, unsigned long long *out, hipStream_t st);
// V-plot over ranges of one width (bsig_plan_create_vplot).  k_vplot_tiles: run r = count tiles [runs[r].x, runs[r].y), a frag
// plan's; every workgroup ADDS into out (n_rows x n_cols int64, row-major): zero `out` first.  P.div_magic / P.div_shift
// divide by lenbin, bin_magic / bin_shift by binsize (magic_u31's; either unused where the divisor is 1).  global: one 64-bit
// global atomic per accepted read; else a table of 32-bit counters in LDS, flushed at the run's end, which must fit
// lds_budget bytes (the filter table joins it there while the two fit).  merge: equal cells of a wave are merged before the
// atomic.  windows / resolve_first as in launch_sum_tiles (no fixed windows).
TileForm vplot_form(int threads, bool global, bool merge, int n_cells, size_t lds_budget);
hipError_t launch_vplot_tiles(int threads, bool global, bool merge, size_t lds_budget, const BsigReadsDev &R, const BsigKParams &P,
                              const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                              bool resolve_first, int n_rows, int n_cols, int lenbin, int binsize, uint32_t bin_magic, int bin_shift,
                              unsigned long long *out, hipStream_t st);
// Depth histogram over ranges (bsig_plan_create_hist).  k_hist_tiles: run r = per-base tiles [runs[r].x, runs[r].y) of 5' ends
// (P.ss: every (base, strand) a cell; else the strands' sum) or of coverage; every workgroup ADDS its non-zero rows into out
// (n_rows int64: row min(value, n_rows - 1)), then the sum of the values into out[n_rows + 1]; the first workgroup adds
// n_cells, the plan's count of cells, to out[n_rows]: zero `out` first.  wide: 32-bit image cells for the tiles with more
// reads than a 16-bit cell may see (tiles flagged BSIG_ITEM_HEAVY are skipped by the launch that is not wide).  merge:
// zero cells counted by ballot, equal rows of a wave merged before the LDS atomic.  half: the form for P.packed_half.
// windows / resolve_first as in launch_sum_tiles (no fixed windows).
TileForm hist_form(int threads, bool coverage, bool half, bool wide, bool merge, int tile_cells, int n_rows);
hipError_t launch_hist_tiles(int threads, bool coverage, bool wide, bool merge, const BsigReadsDev &R, const BsigKParams &P,
                             const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                             bool resolve_first, int n_rows, unsigned long long n_cells, unsigned long long *out, hipStream_t st);
// Per-range summaries (bsig_plan_create_summary).  k_summary_tiles: run r = per-base tiles [runs[r].x, runs[r].y) as
// k_hist_tiles walks them; a tile's out_off is its range's first result row (range x S, S = 2 for 5' ends with P.ss).  Every
// workgroup ADDS into row q of out, 3 + T.k int64 a row: [0] the cells' sum, [3 + j] the cells >= T.t[j], and takes the MAX
// of [1] with the key value << 32 | (2^32 - 1 - cell): zero `out` first, launch_summary_finish last ([1] max, [2] summit, -1
// for a row no tile wrote).  T.t past T.k must be 2^32 - 1.  wide / half / windows / resolve_first as in launch_hist_tiles.
TileForm summary_form(int threads, bool coverage, bool half, bool wide, int tile_cells);
hipError_t launch_summary_tiles(int threads, bool coverage, bool wide, const BsigReadsDev &R, const BsigKParams &P,
                                const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                                bool resolve_first, const BsigThresholds &T, unsigned long long *out, hipStream_t st);
hipError_t launch_summary_finish(int64_t n_rows, int stride, long long *out, hipStream_t st);
// Scaled regions (bsig_plan_create_scaled).  k_scaled_tiles: runs, tiles and out_off (the range's first result row) as for
// launch_summary_tiles; a row of out is n_bins int64, and every workgroup ADDS the cells of a tile into the bins
// floor(c * n_bins / w) of its range's row(s): zero `out` first.  segmented: the wave sums the lanes of one bin before the
// LDS add (16-bit images only; a wide launch ignores it).  wide / half / windows / resolve_first as in launch_hist_tiles.
TileForm scaled_form(int threads, bool coverage, bool half, bool wide, bool segmented, int tile_cells, int rows, int n_bins);
hipError_t launch_scaled_tiles(int threads, bool coverage, bool wide, bool segmented, const BsigReadsDev &R, const BsigKParams &P,
                               const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                               bool resolve_first, int n_bins, unsigned long long *out, hipStream_t st);
// Capped 5' ends (bsig_plan_create_capped).  k_capped_tiles: runs and per-base tiles as for launch_hist_tiles, of a plan whose
// image is strand-split (P.ss = 1, P.binsize = 1); a tile's out_off is its RANGE's first cell of the int32 result, which is
// in bsig_layout's order for the call's bins and ss_out.  Every 5'-end cell is capped at keep_dup per strand.  binned false:
// bins of one base, every tile stores its own cells.  binned true: cell c of a range goes to bin __umulhi(c, bin_magic) >>
// bin_shift (magic_u31's; bamCount: one bin of 2^31 - 1 bases) through n_acc int32 LDS accumulators a row (planmath.h:
// capped_tile_bins) and every workgroup ADDS into out: zero `out` first.  wide / half / windows / resolve_first as in
// launch_hist_tiles.
TileForm capped_form(int threads, bool half, bool wide, bool binned, int tile_cells, int rows, int n_acc);
hipError_t launch_capped_tiles(int threads, bool wide, bool binned, const BsigReadsDev &R, const BsigKParams &P,
                               const BsigWorkItem *items, int64_t n_items, const uint2 *runs, int64_t n_runs, void *windows,
                               bool resolve_first, int keep_dup, int ss_out, uint32_t bin_magic, int bin_shift, int n_acc,
                               int32_t *out, hipStream_t st);
// Capped coverage, stage 2 (capped.hip).  scratch: per range a row of slen (forward, reverse) pairs of capped 5' ends in genome
// order, as launch_capped_tiles stores them for the widened '+' ranges (ss_out 1, not binned).  launch_capped_scan: every row's
// inclusive prefix sums in place (uint32, modulo 2^32).  launch_capped_cover: the coverage of reads resized to frag_len bases
// from those, cell x of a range to bin __umulhi(x, bin_magic) >> bin_shift of its result cells (ss: 2 * bin + antisense);
// binned false: bins of one base, stored; binned true: ADDED -- zero `out` first.  One workgroup per range.
hipError_t launch_capped_scan(const BsigCappedRange *ranges, int64_t n_ranges, uint32_t *scratch, hipStream_t st);
hipError_t launch_capped_cover(const BsigCappedRange *ranges, int64_t n_ranges, const uint32_t *scratch, int frag_len, int ss,
                               bool binned, uint32_t bin_magic, int bin_shift, int32_t *out, hipStream_t st);
hipError_t warm_pileup_module(hipStream_t st);
hipError_t launch_visits(const BsigReadsDev &R, const BsigKParams &P, int mode, const BsigWorkItem *items,
                         int64_t n_items, unsigned long long *acc, hipStream_t st);

}  // namespace bsig
#endif
