// Internals shared by the host runtime (runtime.hip) and the device-side BAM decode (devdecode.hip).
#ifndef BSIG_RUNTIME_INTERNAL_H
#define BSIG_RUNTIME_INTERNAL_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/bamsignals_abi.h"
#include "bsig_types.h"
#include "host_util.h"
#include "planmath.h"

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? BSIG_ERR_NOMEM : BSIG_ERR_DEVICE,          \
                        "HIP error %d (%s) at %s:%d: %s", (int)e_, hipGetErrorString(e_),     \
                        __FILE__, __LINE__, #expr);                                            \
    } while (0)

namespace bsig {
// Large device blocks are kept and reused instead of going back to the driver.  Measured on MI355X / ROCm 7.2
// with plain hipMalloc / hipFree (scripts/hipmalloc_stalls.py): a hipMalloc normally returns in 0.3 ms, but
// once about 70 GB have been freed since the last time, ONE hipMalloc takes 2.2-3.4 s (the freed memory is
// handed back in bulk).  A decode of the north star's BAM allocates and frees 25 GB of scratch, so every third
// cold decode of a session paid that.  Blocks of kBlockCacheMin bytes or more therefore come from, and
// return to, a per-process cache of free blocks (best fit within `max_waste`), bounded by env
// BAMSIGNALS_SCRATCH_CACHE_GB per GPU (default 48; above it the largest free blocks are released first);
// bsig_cache_clear() releases all of it.
constexpr size_t kBlockCacheMin = (size_t)1 << 20;
constexpr size_t kSlabBytes = (size_t)1 << 20;       // what a pool carves its small allocations out of
// Every trip into the driver's allocator (hipMalloc, hipFree, hipHostMalloc, hipHostFree) goes through these and
// is metered, per process: where a call's time goes when it is not in a kernel or a copy is then a number
// (bsig_last_call_timing_ex) instead of a guess.
struct AllocMeter {
    std::atomic<int64_t> ns{0}, calls{0};
};
extern AllocMeter g_alloc_meter;
struct AllocTimer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~AllocTimer()
    {
        g_alloc_meter.ns.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
        g_alloc_meter.calls.fetch_add(1);
    }
};
inline hipError_t metered_malloc(void **p, size_t bytes) { AllocTimer t; return hipMalloc(p, bytes); }
inline hipError_t metered_free(void *p) { AllocTimer t; return hipFree(p); }
inline hipError_t metered_host_malloc(void **p, size_t bytes) { AllocTimer t; return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline hipError_t metered_host_free(void *p) { AllocTimer t; return hipHostFree(p); }
// Two page-locked halves of at least `bytes` each, one pair per GPU, for whoever moves bulk data through the host on
// that GPU: the streamed decode on the way in, the result download on the way out.  Pinning 2 x 32 MB costs 10 ms, and
// a session's first call used to pay it once for each.  The holder keeps `mu` for as long as it uses the halves.
struct PinnedPair {
    std::mutex mu;
    uint8_t *buf[2] = {nullptr, nullptr};
    size_t cap = 0;
    int ensure(size_t bytes);          // (holding mu; the device current)
};
PinnedPair &pinned_pair_for(int device);
// *got receives the block's real size (>= bytes), which block_free wants back
hipError_t block_alloc(int device, size_t bytes, double max_waste, void **p, size_t *got);
void block_free(int device, void *p, size_t bytes);
void block_cache_release();
// env BAMSIGNALS_ARENA_GB > 0: one allocation of that size made with the first context of a device; block_alloc
// carves out of it first (runtime.hip)
void arena_reserve(int device);
}  // namespace bsig

// owns a set of device allocations (all of them through block_alloc: the arena if there is one, the cache of
// free blocks for large ones, hipMalloc otherwise).  Requests below kSmall bytes are carved out of slabs of
// kSlabBytes (which the cache of free blocks keeps between uses): a layout or a plan makes a dozen
// allocations of a few hundred bytes each, and every one of them would be a trip into the driver.
// A pool may adopt a RESERVATION: one block made ahead of time (reads_from_bam_device reserves the resident
// columns on a side thread while the file is still being inflated); allocations are carved out of it while
// it lasts.
struct DevPool {
    struct Blk { void *p; size_t bytes; int device; };
    std::vector<Blk> blks;
    int64_t bytes = 0;
    double max_waste;                 // how much larger than asked a cached block may be (long-lived data: little)
    static constexpr size_t kSmall = (size_t)256 << 10;
    uint8_t *slab = nullptr;          // current slab for small requests (one of blks)
    size_t slab_left = 0;
    uint8_t *res = nullptr;           // the adopted reservation (one of blks)
    size_t res_left = 0;
    explicit DevPool(double waste = 1.125) : max_waste(waste) {}
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    void adopt(int device, void *p, size_t got)
    {
        blks.push_back(Blk{p, got, device});
        res = (uint8_t *)p;
        res_left = got;
    }
    // own_block: never out of a slab -- a block of the request's size, which footprint() (and so hbm_bytes) then shows
    // whatever the size.  make_packed_half asks for it when the block holds class-0/1 columns, so a layout with them and
    // one without differ in hbm_bytes even where the packed column alone would fit a slab; a pool that still has room
    // in an adopted reservation carves the block out of that, and footprint() shows nothing either way
    template <typename T>
    hipError_t alloc(T **p, size_t count, bool own_block = false)
    {
        const size_t nbytes = (std::max<size_t>(count * sizeof(T), 16) + 255) & ~(size_t)255;
        bytes += (int64_t)nbytes;
        if (res && nbytes <= res_left) {
            *p = (T *)res;
            res += nbytes;
            res_left -= nbytes;
            return hipSuccess;
        }
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) { *p = nullptr; return e; }
        if (nbytes <= kSmall && !own_block) {
            if (nbytes > slab_left) {
                void *q = nullptr;
                size_t got = 0;
                e = bsig::block_alloc(dev, bsig::kSlabBytes, 2.0, &q, &got);
                if (e != hipSuccess) { *p = nullptr; return e; }
                blks.push_back(Blk{q, got, dev});
                slab = (uint8_t *)q;
                slab_left = got;
            }
            *p = (T *)slab;
            slab += nbytes;
            slab_left -= nbytes;
            return hipSuccess;
        }
        void *q = nullptr;
        size_t got = 0;
        e = bsig::block_alloc(dev, nbytes, max_waste, &q, &got);
        if (e != hipSuccess) { *p = nullptr; return e; }
        blks.push_back(Blk{q, got, dev});
        *p = (T *)q;
        return hipSuccess;
    }
    // device bytes this pool holds (slabs and an over-sized reservation included: what the cache budgets count)
    int64_t footprint() const
    {
        int64_t t = 0;
        for (const Blk &b : blks) t += (int64_t)b.bytes;
        return t;
    }
    void release()
    {
        for (const Blk &b : blks) bsig::block_free(b.device, b.p, b.bytes);
        blks.clear();
        bytes = 0;
        slab = res = nullptr;
        slab_left = res_left = 0;
    }
    ~DevPool() { release(); }
};

struct bsig_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    bool warm_pending = false;
};

struct bsig_reads {
    bsig_ctx *ctx = nullptr;
    BsigReadsDev dev{};
    DevPool pool;
    bsig_reads_info info{};
    int32_t n_ref = 0;
    uint64_t col_cap[BSIG_MAX_CLASSES] = {};      // elements allocated per class column
    uint64_t idx_entries[BSIG_MAX_CLASSES] = {};  // entries allocated per class index
    std::vector<uint32_t> fmtab;                  // host copy of dev.fmtab (BSIG_PACK_CODES entries, or empty)
    std::vector<uint32_t> ref_unit0, ref_units;
    std::vector<int32_t> ref_len;
    // which layout this is: a number no other layout of the process has (next_layout_gen(), taken whenever the resident
    // columns and indexes are (re)built or loaded).  A plan's cached tile windows are valid for exactly one layout.
    uint64_t layout_gen = 0;
    // the rows are aligned blocks of reads split at their N gaps (splice.hip), not reads: only plain coverage may be asked
    bool spliced = false;
    // a spliced set's junction table (junctions.hip): one row per gap of a read, stably sorted by (reference, start, end);
    // the columns live in `pool`.  A plain set has none
    struct Junctions {
        int64_t n = 0;                                   // rows
        const int32_t *start = nullptr, *end = nullptr;  // first and last base of the gap
        const uint32_t *fm = nullptr;                    // the read's flag | mapq << 16
        const int32_t *anchor = nullptr;                 // min(aligned bases left of the gap, right of it)
        const int64_t *ref_off = nullptr;                // device: the first row of every reference, n_ref + 1 entries
        std::vector<int64_t> h_ref_off;                  // ... on the host
    } junc;
    // a spliced set's read table (splice.hip keeps it, genecounts.hip reads it): the reads in BAM order with their blocks as
    // k_block_emit wrote them, before the sort forgets which read a block came from; the columns live in `pool`.  Read i
    // owns blocks blk_off[i] .. blk_off[i + 1] (ascending, disjoint).  An empty spliced set has an empty table (n = 0, the
    // offsets all 0), a plain set has none
    struct ReadTable {
        int64_t n = 0, n_blocks = 0;                     // reads, blocks
        const uint32_t *blk_off = nullptr;               // n + 1 entries
        const uint32_t *fm = nullptr;                    // flag | mapq << 16
        const int32_t *bstart = nullptr, *bend = nullptr;    // first and last base of every block
        const int64_t *ref_off = nullptr;                // device: the first read of every reference, n_ref + 1 entries
        std::vector<int64_t> h_ref_off;                  // ... on the host
    } rtab;
    // a set with bases (nucleotides.hip): an ordinary plain set that also keeps, in `pool`, its reads in BAM order with
    // their CIGARs, bases and qualities -- the BASE TABLE the nucleotide counts walk.  Read k owns operations cig_off[k] ..
    // cig_off[k + 1] and bases seq_off[k] .. seq_off[k + 1]; base g is nibble g of seq (byte g / 2, the high half where g is
    // even) and byte g of qual.  endmax is the running maximum, within the read's reference, of the reads' last bases
    // (clamped to int32): non-decreasing, so both ends of a tile's read window are binary searches.  An empty set with bases
    // has an empty table (present, n = 0); a plain or spliced set has none
    struct BaseTable {
        bool present = false;
        int64_t n = 0, n_ops = 0, n_bases = 0;
        const int32_t *pos = nullptr, *endmax = nullptr;
        const uint32_t *fm = nullptr;                    // flag | mapq << 16
        const int64_t *cig_off = nullptr, *seq_off = nullptr;    // n + 1 entries each
        const uint32_t *cigar = nullptr;
        const uint8_t *seq = nullptr, *qual = nullptr;
        const int64_t *ref_off = nullptr;                // device: the first read of every reference, n_ref + 1 entries
    } btab;
};
namespace bsig { uint64_t next_layout_gen(); }

namespace bsig {
struct BaiIndex;
// what bsig_reads_upload and bsig_reads_upload_spliced ask of the caller's columns (runtime.hip)
int check_columns(const bsig_columns *cols);
// Builds the resident HBM layout of R (span classes + bucket indexes, bsig_types.h) from device
// columns of n reads in BAM order; ref_off is a host array of n_ref + 1 entries.  The input
// columns are only read.
int layout_from_device(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int32_t *ref_len,
                       const int64_t *ref_off, const int32_t *d_pos, const int32_t *d_end,
                       const uint16_t *d_flag, const uint8_t *d_mapq, const int32_t *d_tlen);
// first launches of a process load each source file's code object onto the device: done with the context
hipError_t warm_decode_module(hipStream_t st);      // devdecode.hip
hipError_t warm_collect_module(hipStream_t st);     // collect.hip
// hands the device-side decode's cached scratch back to the driver (devdecode.hip)
void release_decode_scratch();
// the calling thread's last whole-file decode: bytes reserved ahead of time for the resident columns, and the
// seconds the layout waited for that reservation (devdecode.hip)
void decode_reservation_info(double *bytes, double *wait_s);
// > 0: the file (or this build's limits) needs another decode path; nothing was allocated
constexpr int kNeedsCpuPath = 1;
// Whole BAM -> resident reads on every listed GPU: each GPU decodes one share of the BGZF blocks, the
// column shares are all-gathered over xGMI (devdecode.hip).  BSIG_OK, kNeedsCpuPath or an error.
int reads_from_bam_sharded(const std::vector<bsig_ctx *> &ctxs, const std::string &path, int threads,
                           std::vector<bsig_reads *> &out, const char **transport);
// Index-driven decode with several GPUs: the merged BAI islands of the regions [beg, end) are dealt to the
// GPUs in contiguous runs, the column shares all-gathered (devdecode.hip).  BSIG_OK, kNeedsCpuPath or an error.
int reads_from_regions_sharded(const std::vector<bsig_ctx *> &ctxs, const std::string &path, const BaiIndex &idx, int64_t n_regions,
                               const int32_t *rid, const int64_t *beg, const int64_t *end, int threads,
                               std::vector<bsig_reads *> &out, const char **transport);
// a device buffer to (pageable or page-locked) host memory, staged through page-locked halves where
// that is faster (runtime.hip)
int download_to_host(bsig_ctx *ctx, const void *src_dev, void *dst_host, size_t bytes);
// Where a call's result goes in host memory: ONE flat buffer (range i at flat + off[i]), or one destination per
// range (ptrs[i]: the payload of the R vector allocateList made for range i, ref: src/bamsignals.cpp:172-190).
// `off` (n + 1 entries) is the flat layout either way.
struct HostDest {
    int32_t *flat = nullptr;
    int32_t *const *ptrs = nullptr;
    const int64_t *off = nullptr;
    int64_t n = 0;
    int32_t *range(int64_t i) const { return flat ? flat + off[i] : ptrs[i]; }
    // cells [c0, c0 + count) of the flat layout, wherever their ranges live
    void put(int64_t c0, const int32_t *src, int64_t count) const;
};
// a device buffer of `cells` int32 in the flat layout to the destination (runtime.hip)
int download_to_dest(bsig_ctx *ctx, const int32_t *src_dev, const HostDest &dst, int64_t cells);
// ... a slice of the result: `cells` int32 at src_dev belong at cell dst_cell0 of the flat layout.  copy_threads
// host threads move the page-locked halves on (0: the default, env BAMSIGNALS_COPY_THREADS)
int download_slice_to_dest(bsig_ctx *ctx, const int32_t *src_dev, const HostDest &dst, int64_t dst_cell0, int64_t cells, int copy_threads);
// ... several slices as ONE pipelined stream: slice k = cells[k] int32 at src_dev + src_c0[k], bound for cell dst_c0[k]
int download_slices_to_dest(bsig_ctx *ctx, const int32_t *src_dev, int64_t n_slices, const int64_t *src_c0, const int64_t *dst_c0,
                            const int64_t *cells, const HostDest &dst, int copy_threads);
// bsig_plan_run (a plain plan's int32 result) into the plan's own device buffer, then the download to the host.  async:
// the copy is only enqueued.  With timers the kernels are waited for first and the two stages timed apart; without them
// nothing waits between kernels and download.  The caller has checked that p is a plain plan (runtime.hip)
int plan_run_to_host(bsig_plan *p, const HostDest *dst, bool async = false, double *t_kernels = nullptr, double *t_download = nullptr);
// ... and a reduction plan's (sum, xcorr, frag, hist, summary, scaled, vplot; capped): its kind's device run call into the plan's own
// buffer (made at the first call) of the kind's cells -- int64, a capped plan's int32 --, then the download; timed as above.  A
// sum plan without cells has nothing to run
int plan_run_reduced_to_host(bsig_plan *p, void *host, double *t_kernels = nullptr, double *t_download = nullptr);
// (PlanRule, bsig_params as every entry point reads them: planmath.h)
// frag_len: what a resized plan's creator was given (resized_rule has judged it), 0 for every other plan
int check_params(const bsig_params &prm, int64_t n, const int32_t *len, PlanRule *out, int32_t frag_len = 0);
// what only a resized plan asks, ahead of check_params (runtime.hip: resized_rule): a coverage mode, no paired-end
// extension, 1 <= frag_len <= BSIG_FRAG_LEN_MAX
int resized_rule(const bsig_params &prm, int32_t frag_len);
// what only a sum over ranges asks (runtime.hip: sum_shape)
struct SumShape {
    bsig_params tiles;      // the per-base plan the sum is built on
    int32_t width;          // every range's width
    int32_t binsize;        // the caller's bins (the per-base sums are binned at the end: binning is linear)
    int nw;                 // waves per k_sum_tiles workgroup
    int64_t cells;          // ceil(width / binsize), twice that with strands
};
int sum_shape(const bsig_params &prm, int64_t n, const int32_t *len, SumShape *out);
// what only a strand cross-correlation asks, ahead of check_params (runtime.hip: xcorr_shape): max_lag in range, a
// stranded per-base profile without shift or midpoint
struct XcorrShape {
    bsig_params tiles;      // the per-base, strand-split plan the tiles are piled up by
    int32_t max_lag;
    int32_t body;           // body cells of a tile at most (the caller's tile_cells, or the default)
    int64_t cells;          // max_lag + 1 + BSIG_XCORR_MOMENTS
};
int xcorr_shape(const bsig_params &prm, int32_t max_lag, XcorrShape *out);
// what only a fragment-length histogram asks, ahead of check_params (runtime.hip: frag_shape): bamCount's tiles, no shift,
// a length filter, a row width >= 1, at most BSIG_FRAG_MAX_ROWS rows
struct FragShape {
    bsig_params tiles;      // the unstranded count plan the tiles are walked by
    int32_t len_bin;        // lengths per row
    int64_t cells;          // rows: tlen_filter[1] / len_bin + 1
};
int frag_shape(const bsig_params &prm, int32_t len_bin, FragShape *out);
// what only a V-plot asks, ahead of check_params (runtime.hip: vplot_shape): bamProfile without shift or strands, a length
// filter, len_bin and binsize >= 1, ranges of one width (sum_shape's rule), at most BSIG_FRAG_MAX_ROWS rows and
// BSIG_VPLOT_MAX_CELLS cells
struct VplotShape {
    bsig_params tiles;      // the unstranded count plan the tiles are walked by (a frag plan's)
    int32_t len_bin;        // lengths per row
    int32_t binsize;        // positions per column
    int32_t rows, cols;     // tlen_filter[1] / len_bin + 1; ceil(width / binsize), 0 without ranges or width
    int64_t cells;          // rows * cols
};
int vplot_shape(const bsig_params &prm, int64_t n, const int32_t *len, int32_t len_bin, VplotShape *out);
// what only a depth histogram asks, ahead of check_params (runtime.hip: hist_shape): per-base 5' ends or plain coverage, no
// shift, 1 <= max_value < BSIG_HIST_MAX_ROWS, threads and tile_cells the kernel's LDS holds
struct HistShape {
    bsig_params tiles;      // the per-base plan the tiles are piled up by (threads and tile_cells resolved)
    int32_t max_value;      // V: the overflow row
    int64_t cells;          // V + 1 + BSIG_HIST_MOMENTS
};
int hist_shape(const bsig_params &prm, int32_t max_value, HistShape *out);
// what only the per-range summaries ask, ahead of check_params (runtime.hip: summary_shape): the depth histogram's parameter
// rule, and 0 .. BSIG_SUMMARY_MAX_THRESHOLDS thresholds rising from 1
struct SummaryShape {
    bsig_params tiles;      // the per-base plan the tiles are piled up by (threads and tile_cells resolved)
    int S;                  // rows per range: 2 for 5' ends with strands
    int32_t n_thresholds;
    int32_t thresholds[BSIG_SUMMARY_MAX_THRESHOLDS];
    int32_t row;            // int64 per (range, row): BSIG_SUMMARY_FIXED + n_thresholds
};
int summary_shape(const bsig_params &prm, int32_t n_thresholds, const int32_t *thresholds, SummaryShape *out);
// what only the scaled regions ask, ahead of check_params (runtime.hip: scaled_shape): the depth histogram's parameter rule,
// and 1 .. BSIG_SCALED_MAX_BINS bins
struct ScaledShape {
    bsig_params tiles;      // the per-base plan the tiles are piled up by (threads and tile_cells resolved)
    int S;                  // rows per range: 2 for 5' ends with strands
    int32_t n_bins;         // N: int64 per (range, row)
};
int scaled_shape(const bsig_params &prm, int32_t n_bins, ScaledShape *out);
// what only a capped plan asks, ahead of check_params (runtime.hip: capped_shape): single ends (no midpoint, no extension, no
// template-length rule), keep_dup >= 1, threads and tile_cells the kernel's LDS holds; frag_len 0 on bamProfile or bamCount
// (the capped 5' ends), 1 .. BSIG_FRAG_LEN_MAX on bamCoverage (the capped coverage of resized reads)
struct CappedShape {
    bsig_params tiles;      // the per-base, strand-split 5'-end plan the tiles are piled up by (threads and tile_cells resolved)
    int32_t keep_dup;       // k: every (base, strand) cell counts min(cell, k)
    int32_t frag_len;       // 0, or the bases every kept read covers from its 5' end
    int32_t lay_binsize;    // bsig_layout's binsize of the RESULT (-1: bamCount)
    int32_t binsize;        // the bins the kernels divide by (planmath.h: capped_binsize)
    int S;                  // values per result cell: 2 with strands
    // the capped coverage: the plan's tiles walk the WIDENED ranges (planmath.h: capped_widen), all of them as '+' ranges;
    // these are the caller's own widths and strands and every widened range's lead (bsig_plan_create_capped fills them)
    const int32_t *len0 = nullptr, *strand0 = nullptr, *lead = nullptr;
};
int capped_shape(const bsig_params &prm, int32_t keep_dup, int32_t frag_len, CappedShape *out);
// BSIG_ERR_ARG if the plan's last run took a coverage bin past INT32_MAX (bsig_plan_overflowed), else BSIG_OK;
// for callers that have synchronised the plan's stream
int plan_check_overflow(bsig_plan *p);
// widest coverage bin: a tile that is not cut into slices (at most 32,767 reads) cannot take a bin past INT32_MAX
constexpr int32_t kMaxCoverageBin = 65536;
}  // namespace bsig
#endif
