// Host runtime behind include/bamsignals_abi.h: device context, reads resident in HBM,
// plans (ranges + parameters -> work items) and their execution on a HIP stream.
//
// There is no CPU fallback in this library: every compute entry point needs a gfx950 device
// and fails with BSIG_ERR_DEVICE otherwise.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <numeric>
#include <thread>
#include <string>
#include <vector>

#include "../../include/bamsignals_abi.h"
#include "bsig_types.h"
#include "host_util.h"
#include "kernels.h"

namespace bsig {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace bsig

using bsig::fail;

#include "runtime_internal.h"

// ---------------------------------------------------------------------------------------------
// the per-process cache of large free device blocks (runtime_internal.h)
// ---------------------------------------------------------------------------------------------
namespace bsig {
AllocMeter g_alloc_meter;
namespace {
struct BlockCache {
    struct Blk { int dev; void *p; size_t bytes; };
    std::mutex mu;
    std::vector<Blk> free_;
    size_t cached = 0;
} g_blocks;
size_t block_cache_limit()
{
    size_t gb = 48;
    if (const char *e = getenv("BAMSIGNALS_SCRATCH_CACHE_GB")) gb = (size_t)std::max(0ll, atoll(e));
    return gb << 30;
}
}  // namespace

// ---- an arena reserved with the context (env BAMSIGNALS_ARENA_GB, default 0 = none) -------------------------
// Every hipMalloc is a trip into the driver, and on a shared host those trips are where a call's time goes
// astray (the stalls above; 0.1-0.5 s extra in the walk and the layout of one cold call in four on a busy
// box).  With an arena ONE allocation is made when the context comes up; blocks are carved out of it (first
// fit, 4-KiB aligned, neighbours merged again when they come back) and a cold call makes no allocation at all
// as long as its scratch and its resident reads fit.  What does not fit takes the paths above.
namespace {
struct Arena {
    int dev = -1;
    uint8_t *base = nullptr;
    size_t size = 0;
    std::vector<std::pair<size_t, size_t>> free_;      // (offset, length), sorted by offset, never adjacent
};
std::mutex g_arena_mu;
std::vector<Arena> g_arenas;
Arena *arena_of(int device)
{
    for (Arena &a : g_arenas)
        if (a.dev == device) return &a;
    return nullptr;
}
bool arena_take(int device, size_t bytes, void **p, size_t *got)
{
    std::lock_guard<std::mutex> lk(g_arena_mu);
    Arena *a = arena_of(device);
    if (!a) return false;
    const size_t need = (bytes + 4095) & ~(size_t)4095;
    for (size_t k = 0; k < a->free_.size(); ++k) {
        if (a->free_[k].second < need) continue;
        *p = a->base + a->free_[k].first;
        *got = need;
        a->free_[k].first += need;
        a->free_[k].second -= need;
        if (a->free_[k].second == 0) a->free_.erase(a->free_.begin() + (long)k);
        return true;
    }
    return false;
}
bool arena_give(int device, void *p, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_arena_mu);
    Arena *a = arena_of(device);
    if (!a || (uint8_t *)p < a->base || (uint8_t *)p >= a->base + a->size) return false;
    const size_t off = (size_t)((uint8_t *)p - a->base);
    auto it = std::lower_bound(a->free_.begin(), a->free_.end(), std::make_pair(off, (size_t)0));
    it = a->free_.insert(it, {off, bytes});
    if (it + 1 != a->free_.end() && it->first + it->second == (it + 1)->first) { it->second += (it + 1)->second; a->free_.erase(it + 1); }
    if (it != a->free_.begin() && (it - 1)->first + (it - 1)->second == it->first) { (it - 1)->second += it->second; a->free_.erase(it); }
    return true;
}
}  // namespace

void arena_reserve(int device)
{
    const char *e = getenv("BAMSIGNALS_ARENA_GB");
    const long long gb = e ? atoll(e) : 0;
    if (gb <= 0) return;
    std::lock_guard<std::mutex> lk(g_arena_mu);
    if (arena_of(device)) return;
    Arena a;
    a.dev = device;
    a.size = (size_t)gb << 30;
    if (hipSetDevice(device) != hipSuccess || metered_malloc((void **)&a.base, a.size) != hipSuccess) { (void)hipGetLastError(); return; }
    a.free_.push_back({0, a.size});
    g_arenas.push_back(a);
}

// (bsig_cache_clear: an arena nobody holds a block of goes back to the driver)
static void arena_release_idle()
{
    std::lock_guard<std::mutex> lk(g_arena_mu);
    for (size_t k = 0; k < g_arenas.size();) {
        Arena &a = g_arenas[k];
        if (a.free_.size() == 1 && a.free_[0].first == 0 && a.free_[0].second == a.size) {
            (void)hipSetDevice(a.dev);
            (void)metered_free(a.base);
            g_arenas.erase(g_arenas.begin() + (long)k);
        } else {
            ++k;
        }
    }
}

hipError_t block_alloc(int device, size_t bytes, double max_waste, void **p, size_t *got)
{
    if (arena_take(device, std::max<size_t>(bytes, 256), p, got)) return hipSuccess;
    bytes = (std::max<size_t>(bytes, 256) + 255) & ~(size_t)255;
    if (bytes >= kBlockCacheMin) {
        std::lock_guard<std::mutex> lk(g_blocks.mu);
        size_t best = (size_t)-1;
        const size_t cap = (size_t)((double)bytes * max_waste) + (1u << 20);
        for (size_t k = 0; k < g_blocks.free_.size(); ++k) {
            const BlockCache::Blk &b = g_blocks.free_[k];
            if (b.dev != device || b.bytes < bytes || b.bytes > cap) continue;
            if (best == (size_t)-1 || b.bytes < g_blocks.free_[best].bytes) best = k;
        }
        if (best != (size_t)-1) {
            *p = g_blocks.free_[best].p;
            *got = g_blocks.free_[best].bytes;
            g_blocks.cached -= g_blocks.free_[best].bytes;
            g_blocks.free_.erase(g_blocks.free_.begin() + (long)best);
            return hipSuccess;
        }
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = metered_malloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        // the cache itself may be what fills the device: hand it back and try once more
        (void)hipGetLastError();
        block_cache_release();
        (void)hipSetDevice(device);
        e = metered_malloc(p, bytes);
    }
    if (e != hipSuccess) { *p = nullptr; return e; }
    *got = bytes;
    return hipSuccess;
}

void block_free(int device, void *p, size_t bytes)
{
    if (!p) return;
    if (arena_give(device, p, bytes)) return;
    if (bytes < kBlockCacheMin) {                     // small blocks are not worth keeping
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != device) (void)hipSetDevice(device);
        (void)metered_free(p);
        if (cur != device) (void)hipSetDevice(cur);
        return;
    }
    const size_t limit = block_cache_limit();          // per device: every GPU has its own HBM
    std::vector<BlockCache::Blk> drop;
    {
        std::lock_guard<std::mutex> lk(g_blocks.mu);
        g_blocks.free_.push_back(BlockCache::Blk{device, p, bytes});
        g_blocks.cached += bytes;
        for (;;) {
            size_t on_dev = 0, big = (size_t)-1;
            for (size_t k = 0; k < g_blocks.free_.size(); ++k) {
                if (g_blocks.free_[k].dev != device) continue;
                on_dev += g_blocks.free_[k].bytes;
                if (big == (size_t)-1 || g_blocks.free_[k].bytes > g_blocks.free_[big].bytes) big = k;
            }
            if (on_dev <= limit || big == (size_t)-1) break;
            drop.push_back(g_blocks.free_[big]);
            g_blocks.cached -= g_blocks.free_[big].bytes;
            g_blocks.free_.erase(g_blocks.free_.begin() + (long)big);
        }
    }
    if (drop.empty()) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const BlockCache::Blk &b : drop) { (void)hipSetDevice(b.dev); (void)metered_free(b.p); }
    (void)hipSetDevice(cur);
}

void block_cache_release()
{
    arena_release_idle();
    std::vector<BlockCache::Blk> all;
    {
        std::lock_guard<std::mutex> lk(g_blocks.mu);
        all.swap(g_blocks.free_);
        g_blocks.cached = 0;
    }
    if (all.empty()) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const BlockCache::Blk &b : all) { (void)hipSetDevice(b.dev); (void)metered_free(b.p); }
    (void)hipSetDevice(cur);
}
}  // namespace bsig

namespace { enum { kSumProfile = 0, kSumCover = 1, kSumCoverSS = 2 }; }      // launch_sum_tiles' kinds (kernels.h)
// What a plan is: a plain one gives every range its own int32 cells; sum, xcorr, frag and hist reduce all ranges to one short
// int64 vector, a summary reduces every range by itself to a few int64, a scaled plan to n_bins int64; a capped plan gives every
// range its own int32 cells, as a plain one does, but runs as the reductions do (runs of tiles walked whole).
// The order is the one the wrong-kind refusals are worded by (wrong_kind).
enum PlanKind { kPlain = 0, kSum, kXcorr, kFrag, kHist, kSummary, kScaled, kVplot, kCapped };
// per kind: the noun with its article, the device run call, the host run call, the bytes of a result cell
struct KindRow { const char *a, *run_dev, *run_host; int cell_bytes; };
static const KindRow kKinds[] = {
    {"a plain", "bsig_plan_run", "bsig_plan_run_host", 4},
    {"a sum", "bsig_plan_run_sum", "bsig_plan_run_sum_host", 8},
    {"an xcorr", "bsig_plan_run_xcorr", "bsig_plan_run_xcorr_host", 8},
    {"a frag", "bsig_plan_run_frag", "bsig_plan_run_frag_host", 8},
    {"a hist", "bsig_plan_run_hist", "bsig_plan_run_hist_host", 8},
    {"a summary", "bsig_plan_run_summary", "bsig_plan_run_summary_host", 8},
    {"a scaled", "bsig_plan_run_scaled", "bsig_plan_run_scaled_host", 8},
    {"a vplot", "bsig_plan_run_vplot", "bsig_plan_run_vplot_host", 8},
    {"a capped", "bsig_plan_run_capped", "bsig_plan_run_capped_host", 4},
};
// A reduction plan's own (every kind but kPlain): the result's cells, the device buffer its _host call runs into, and the
// tiles cut into runs (a workgroup each) -- the main tiles' runs, then the extra ones': a sum plan's heavy slices, an xcorr or
// hist, summary or scaled plan's wide tiles (32-bit image, one tile a run), none for a frag or vplot plan.  Beside them what only one kind has.
struct Reduced {
    int64_t cells = 0;                  // of kKinds[kind].cell_bytes each
    int64_t *d_out = nullptr;           // device result of bsig_plan_run_<kind>_host, kept between calls (whole qwords)
    uint2 *runs = nullptr;              // [t0, t1) of the items, the extra runs of the heavy items
    int64_t n_runs_main = 0, n_runs_extra = 0;
    // sum (bsig_plan_create_sum): per-base tiles ordered by c0, a run of one c0, summed over the ranges by k_sum_tiles
    struct {
        int kind = kSumProfile, S = 1;
        int nw = 0;                     // waves per k_sum_tiles workgroup
        int32_t width = 0, binsize = 1; // every range's width; the caller's bins (the per-base sums are binned at the end)
        BsigSumChunk *chunks = nullptr;
        int64_t n_chunks = 0;
        int32_t max_nvals = 0;
        int32_t slab_vals = 0;          // int32 per slab (tile_cells * S rounded up to 4)
        int32_t *slab = nullptr;        // one slab per run
        long long *base = nullptr;      // per-base sums (binsize > 1; binsize 1 reduces straight into the result)
    } sum;
    // xcorr (bsig_plan_create_xcorr): tiles of body + halo in genomic order
    struct {
        int body = 0;                   // body cells of a tile (the image holds body + max_lag: the plan's tile_cells)
        int max_lag = 0;
        int64_t n_cells = 0;            // moments[0]: the sum of the ranges' widths
    } xcorr;
    // frag (bsig_plan_create_frag): count tiles in genomic order
    struct {
        bool merge = false;             // k_frag_tiles' form: equal rows of a wave merged before the LDS atomic (see frag_setup)
        int32_t len_bin = 1;            // lengths per row
    } frag;
    // hist (bsig_plan_create_hist): per-base tiles in genomic order
    struct {
        bool coverage = false;          // the signal: coverage, else 5' ends
        bool merge = false;             // k_hist_tiles' form: zero cells by ballot, equal rows of a wave merged (see hist_setup)
        int32_t max_value = 0;          // V: the overflow row
        int64_t n_cells = 0;            // moments[0]: the cells of all ranges
    } hist;
    // summary (bsig_plan_create_summary): per-base tiles in genomic order, their out_off the range's first result row
    struct {
        bool coverage = false;          // the signal: coverage, else 5' ends
        int S = 1;                      // rows per range
        BsigThresholds thr{};           // the kernel's argument: K thresholds, the rest 2^32 - 1
    } summary;
    // scaled (bsig_plan_create_scaled): the summary plan's tiles; a result row is n_bins int64
    struct {
        bool coverage = false;          // the signal: coverage, else 5' ends
        int S = 1;                      // rows per range
        int32_t n_bins = 0;             // N
        bool segmented = false;         // the wave sums the lanes of one bin before the LDS add (k_scaled_tiles)
    } scaled;
    // vplot (bsig_plan_create_vplot): a frag plan's count tiles; the result is rows x cols int64, row-major
    struct {
        int32_t rows = 0, cols = 0;     // lengths / len_bin, positions / binsize
        int32_t len_bin = 1, binsize = 1;
        uint32_t bin_magic = 0;         // magic_u31 of binsize (len_bin's is the plan's P.div_magic)
        int32_t bin_shift = 0;
        int form = 0;                   // k_vplot_tiles' form: 0 a table in LDS, 1 global atomics (see vplot_setup)
        bool merge = false;             // ... equal cells of a wave merged before the atomic
        size_t lds_budget = 0;          // bytes of LDS the table may take (decides the form, and where the filter table lives)
    } vplot;
    // capped (bsig_plan_create_capped): per-base strand-split tiles, their out_off the range's first cell of the int32 result
    struct {
        int32_t keep_dup = 1;           // k
        int S = 1;                      // values per result cell
        bool binned = false;            // bins wider than a base, or bamCount: the kernels add into a zeroed result
        uint32_t bin_magic = 0;         // magic_u31 of the bins' width (planmath.h: capped_binsize)
        int32_t bin_shift = 0;
        int32_t n_acc = 0;              // LDS accumulators a row (planmath.h: capped_tile_bins)
        // the capped coverage (frag_len > 0): the tiles store into `scratch` (the plan's off is ITS layout: bins of one base,
        // strands kept, over the widened ranges), k_capped_scan and k_capped_cover make the result, laid out by res_off
        int32_t frag_len = 0;
        uint32_t *scratch = nullptr;
        BsigCappedRange *ranges = nullptr;
        std::vector<int64_t> res_off;   // bsig_layout of the caller's ranges, bins and strands
    } capped;
};

struct bsig_plan {
    bsig_ctx *ctx = nullptr;
    const bsig_reads *reads = nullptr;
    int mode = 0;                  // what the caller asked for (fixes the result layout)
    int kernel_mode = 0;           // which kernel family runs: profile with very wide bins is
                                   // executed as a bamCount over the bins' sub-intervals
    BsigKParams kp{};
    int tile_cells = 0, threads = 0;
    int64_t n_ranges = 0, n_items = 0;
    std::vector<int64_t> off;
    DevPool pool;
    BsigWorkItem *items = nullptr;
    int32_t *d_out = nullptr;      // device result buffer of bsig_plan_run_host, kept between calls
    // slices of heavy tiles (tiles whose read windows hold more reads than probe_windows' heavy_reads): the same
    // kernels run a second time over these items with fixed windows and accumulate = 1
    BsigWorkItem *heavy_items = nullptr;
    void *heavy_windows = nullptr;
    int64_t n_heavy_slices = 0, n_heavy_tiles = 0;
    // count family only: some cells are reached by global atomic adds (sub-intervals of a range wider than
    // one workgroup's share, wide bins) or by no work item at all (zero-width ranges), so the result must
    // be zeroed in front of the launch.  Ranges of one tile store their counters themselves.
    bool needs_zero = false;
    bool have_visits = false;
    unsigned long long visits[BSIG_MAX_CLASSES + 1] = {};      // k_visits' counts (bsig_plan_get_stats), taken once
    uint8_t *ptab = nullptr;            // the packed class's filter table for kp (BsigKParams::ptab)
    int32_t *overflow = nullptr;        // binned coverage with heavy slices: 1 if a run's atomic adds took a bin past INT32_MAX
    BsigResolved *resolved = nullptr;   // large launches: the windows of every tile, written by k_resolve_tiles
    uint64_t resolved_gen = 0;          // ... for this layout of the reads (0: not yet): a later run on the same layout reuses them
    uint64_t made_for_gen = 0;          // the layout the plan was made on: its tiles' heavy slices and the packed class's filter
                                        // table are read off that layout, so a plan does not outlive it
    int64_t runs = 0;                   // runs so far (a plan that is run AGAIN is a resident one: plan_two_launches)
    PlanKind kind = kPlain;
    std::unique_ptr<Reduced> red;       // a reduction plan's own: there if and only if kind != kPlain
};
static int64_t g_resolve_min_override = -1;     // bsig_debug_set_knob(4, n): two launches from n tiles on (sweeps)
// does a run of this plan look its windows up in a launch of its own?  (measured at the north star's read density,
// scripts/ns_variants.py: 15,000 tiles 28.3 us fused / 31.1 us in two launches, 25,000 43.3 / 46.2, 35,000 71.8 / 66.3,
// 50,000 112.0 / 107.3, 100,000 189.7 / 177.1; config 5's share 180.6 / 157.5, config 4's call 407 / 370:
// env BAMSIGNALS_RESOLVE_MIN_TILES, default 32,768)
// are a large launch's tile windows kept with the plan after its first run (default), or looked up in every run?
static bool windows_kept()
{
    const char *e = getenv("BAMSIGNALS_CACHE_WINDOWS");      // (read per run: a test flips it)
    return !(e && !strcmp(e, "0"));
}

static bool plan_two_launches(const bsig_plan *p)
{
    static const int64_t resolve_min = getenv("BAMSIGNALS_RESOLVE_MIN_TILES") ? atoll(getenv("BAMSIGNALS_RESOLVE_MIN_TILES")) : (int64_t)32768;
    // (the count family walks four tiles per wave and looks their windows up side by side: a launch of its own
    // for them measured the same or slower there -- 0.1469 fused, 0.1476 in two launches on config 3's tiling --
    // so bamCount keeps the fused form for a step that pays the lookup; with the windows kept it takes the other
    // from its second run on like everybody: 0.0949 / 0.0975 -> 0.0925 / 0.0945 ms on that tiling)
    if (g_resolve_min_override >= 0) return p->n_items > 0 && p->n_items >= g_resolve_min_override;
    if (p->n_items >= resolve_min && p->kernel_mode != BSIG_MODE_COUNT) return p->n_items > 0;
    // Those figures are for a step that pays the lookup launch.  A plan that is run a second time is a resident one, and
    // with the windows kept its later steps pay nothing for them: from its second run on a plan takes the form for
    // resolved windows whatever its size -- a workgroup's life is one dependent memory trip shorter -- (10,000 tiles: 19.56
    // -> 18.30 us a step; 4,000: 10.08 -> 9.37; 1,500: 6.76 -> 5.57; 400: 5.58 -> 4.62; 100: 5.29 -> 4.35; its second
    // run carries the lookup launch, a plan that is run once -- every file-level call -- never sees it).
    static const int64_t again_min = getenv("BAMSIGNALS_RESOLVE_AGAIN_MIN_TILES") ? atoll(getenv("BAMSIGNALS_RESOLVE_AGAIN_MIN_TILES")) : (int64_t)1;
    return windows_kept() && p->runs >= 1 && p->n_items >= again_min;
}

extern "C" {

int bsig_abi_version(void) { return BSIG_ABI_VERSION; }

const char *bsig_last_error(void) { return bsig::g_last_error.c_str(); }

// allocateList's shapes (ref: src/bamsignals.cpp:139-192)
int64_t bsig_layout(int64_t n, const int32_t *len, int32_t binsize, int32_t ss, int64_t *off)
{
    const int64_t mult = ss ? 2 : 1;
    int64_t acc = 0;
    for (int64_t i = 0; i < n; ++i) {
        off[i] = acc;
        if (binsize <= 0) acc += mult;
        else if (len[i] > 0) acc += mult * (((int64_t)len[i] + binsize - 1) / binsize);
    }
    off[n] = acc;
    return acc;
}

int bsig_device_count(int32_t *n)
{
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail(BSIG_ERR_DEVICE, "no HIP device: %s", hipGetErrorString(e)); }
    *n = c;
    return BSIG_OK;
}

int bsig_ctx_create(int32_t device, void *stream, bsig_ctx **out)
{
    if (!out) return fail(BSIG_ERR_ARG, "ctx output pointer is NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(BSIG_ERR_DEVICE, "no HIP device available (bamsignals_hip has no CPU fallback)");
    if (device < 0 || device >= count) return fail(BSIG_ERR_ARG, "device %d out of range [0,%d)", device, count);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BSIG_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    {
        // the first hipMalloc of a process sets the runtime's allocator up (76 ms measured): that belongs to
        // bringing the device up, not to whichever call happens to allocate first
        void *warm = nullptr;
        if (hipMalloc(&warm, 256) == hipSuccess) (void)hipFree(warm);
        (void)hipGetLastError();
    }
    bsig::arena_reserve(device);
    bsig_ctx *c = new bsig_ctx;
    {
        static std::mutex warm_mu;
        static std::vector<int> warmed;
        std::lock_guard<std::mutex> lk(warm_mu);
        if (std::find(warmed.begin(), warmed.end(), device) == warmed.end()) { warmed.push_back(device); c->warm_pending = true; }
    }
    c->device = device;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return fail(BSIG_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e)); }
        c->owns_stream = true;
    }
    if (c->warm_pending) {
        // ... and so does the first launch out of each code object of this library (walk / extract / inflate,
        // pileup, reassembly): about 10 ms apiece, once per process and device
        (void)bsig::warm_pileup_module(c->stream);
        (void)bsig::warm_decode_module(c->stream);
        (void)bsig::warm_collect_module(c->stream);
        // ... and so do the runtime's own staging buffers for copies from and to pageable memory (the record
        // walk's per-block summaries come back that way)
        {
            void *d = nullptr;
            std::vector<uint8_t> h((size_t)4 << 20, 0);
            if (hipMalloc(&d, h.size()) == hipSuccess) {
                (void)hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, c->stream);
                (void)hipMemcpyAsync(h.data(), d, h.size(), hipMemcpyDeviceToHost, c->stream);
                (void)hipStreamSynchronize(c->stream);
                (void)hipFree(d);
            }
        }
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        c->warm_pending = false;
    }
    *out = c;
    return BSIG_OK;
}

void bsig_ctx_destroy(bsig_ctx *c)
{
    if (!c) return;
    if (c->owns_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bsig_ctx_sync(bsig_ctx *c)
{
    if (!c) return fail(BSIG_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BSIG_OK;
}

void *bsig_ctx_stream(bsig_ctx *c) { return c ? (void *)c->stream : nullptr; }

int bsig_host_alloc(int64_t bytes, void **ptr)
{
    if (!ptr || bytes < 0) return fail(BSIG_ERR_ARG, "bad argument to bsig_host_alloc");
    *ptr = nullptr;
    HIP_TRY(hipHostMalloc(ptr, (size_t)std::max<int64_t>(bytes, 16), hipHostMallocDefault));
    return BSIG_OK;
}

void bsig_host_free(void *ptr)
{
    if (ptr) (void)hipHostFree(ptr);
}

// ---------------------------------------------------------------------------------------------
// reads -> HBM
// ---------------------------------------------------------------------------------------------
}  // extern "C"

// The resident layout from device columns; shared by bsig_reads_upload (host columns) and the
// device-side BAM decode (devdecode.hip).
uint64_t bsig::next_layout_gen()
{
    static std::atomic<uint64_t> g{0};
    return ++g;
}

// The packed class's 16-bit 5'-end column (bsig_types.h: p5h), derived from its words and the pair table wherever a
// bsig_reads is made (laid out, cloned, loaded) and never saved.  +2 bytes per packed read in HBM (R->info.hbm_bytes).
// env BAMSIGNALS_PACKED_HALF=0, read here: no column, every plan reads the 4-byte words.
// Span classes 0 and 1 get the same column (+2 bytes per read of theirs), behind the packed class's in ONE block -- the
// kernels reach them as offsets from the packed column (BsigKParams::short_off: a scalar register each instead of a
// pointer's two) -- unless the class holds a read outside its reference (kernels.hip: k_make_short_p5h).
// env BAMSIGNALS_SHORT_HALF=0, read here as well: the packed class's column only.
static int make_packed_half(bsig_reads *R, hipStream_t st)
{
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) R->dev.cls[c].p5h = nullptr;
    const char *e = getenv("BAMSIGNALS_PACKED_HALF");
    BsigClassCols &C = R->dev.cls[BSIG_CLASS_PACKED];
    if (C.n == 0 || !R->dev.fmtab || (e && !strcmp(e, "0"))) return BSIG_OK;
    const char *es = getenv("BAMSIGNALS_SHORT_HALF");
    auto cap_of = [](int64_t n) { return n ? (n + 7) / 8 * 8 + 8 : (int64_t)0; };     // the 16-B loads of the last reads stay inside, and read zeros
    const int64_t cap = cap_of(C.n);
    int64_t cap_s[2] = {cap_of(R->dev.cls[0].n), cap_of(R->dev.cls[1].n)};
    if ((es && !strcmp(es, "0")) || cap + cap_s[0] + cap_s[1] >= ((int64_t)1 << 32)) cap_s[0] = cap_s[1] = 0;
    uint16_t *p = nullptr;
    HIP_TRY(R->pool.alloc(&p, (size_t)(cap + cap_s[0] + cap_s[1]), cap_s[0] + cap_s[1] != 0));
    HIP_TRY(bsig::launch_make_p5h(C.fm, R->dev.fmtab, C.n, cap, p, st));
    int bad[2] = {0, 0};
    if (cap_s[0] + cap_s[1]) {
        // one small scratch block: the references' first units, their unit counts, the two flags
        const size_t nr = (size_t)R->n_ref;
        uint32_t *d_tab = nullptr;
        HIP_TRY(hipMalloc((void **)&d_tab, (2 * nr + 2) * sizeof(uint32_t)));
        int *d_bad = reinterpret_cast<int *>(d_tab + 2 * nr);
        hipError_t he = hipMemcpyAsync(d_tab, R->ref_unit0.data(), nr * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(d_tab + nr, R->ref_units.data(), nr * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemsetAsync(d_bad, 0, sizeof bad, st);
        for (int c = 0; c < 2 && he == hipSuccess; ++c) {
            const BsigClassCols &S = R->dev.cls[c];
            if (!cap_s[c]) continue;
            he = bsig::launch_make_short_p5h(S.pos, S.fm, c == 0 ? 24 : 20, S.n, cap_s[c], S.idx, R->idx_entries[c] - 2, S.kshift, d_tab,
                                             d_tab + nr, R->n_ref, p + cap + (c ? cap_s[0] : 0), d_bad + c, st);
        }
        if (he == hipSuccess) he = hipMemcpyAsync(bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        (void)hipFree(d_tab);
        HIP_TRY(he);
    } else {
        HIP_TRY(hipStreamSynchronize(st));
    }
    C.p5h = p;
    for (int c = 0; c < 2; ++c)
        if (cap_s[c] && !bad[c]) R->dev.cls[c].p5h = p + cap + (c ? cap_s[0] : 0);
    R->info.hbm_bytes = R->pool.footprint();
    return BSIG_OK;
}

int bsig::layout_from_device(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int32_t *ref_len,
                             const int64_t *ref_off, const int32_t *d_pos, const int32_t *d_end,
                             const uint16_t *d_flag, const uint8_t *d_mapq, const int32_t *d_tlen)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    R->layout_gen = next_layout_gen();          // (whatever a plan cached for an earlier layout of R is stale from here on)

    // global coordinate: references back to back in 64-kbp units
    R->n_ref = n_ref;
    R->ref_unit0.resize(n_ref);
    R->ref_units.resize(n_ref);
    R->ref_len.assign(ref_len, ref_len + n_ref);
    uint64_t total_units = 0;
    for (int r = 0; r < n_ref; ++r) {
        if (ref_len[r] < 0) return fail(BSIG_ERR_ARG, "negative length of reference %d", r);
        const uint64_t u = ((uint64_t)ref_len[r] >> BSIG_REF_UNIT_SHIFT) + 1;
        if (total_units + u >= (1ull << 31)) return fail(BSIG_ERR_ARG, "genome too large for the bucket index");
        R->ref_unit0[r] = (uint32_t)total_units;
        R->ref_units[r] = (uint32_t)u;
        total_units += u;
    }
    const uint64_t total_bp = total_units << BSIG_REF_UNIT_SHIFT;

    R->info = bsig_reads_info{};
    R->info.n_reads = n;
    R->dev.fmtab = nullptr;
    R->dev.n_codes = 0;
    if (n == 0 || n_ref == 0) {
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) R->dev.cls[c] = BsigClassCols{};
        return BSIG_OK;
    }
    DevPool tmp(1e9);          // scratch of this call: any cached block that is large enough will do
    const bool diag = getenv("BSIG_DIAG_DECODE") != nullptr;
    const auto t_diag0 = std::chrono::steady_clock::now();
    auto diag_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_diag0).count(); };
    int64_t *d_ref_off;
    uint32_t *d_unit0, *d_units;
    HIP_TRY(tmp.alloc(&d_ref_off, n_ref + 1));
    HIP_TRY(tmp.alloc(&d_unit0, n_ref));
    HIP_TRY(tmp.alloc(&d_units, n_ref));
    HIP_TRY(hipMemcpyAsync(d_ref_off, ref_off, (n_ref + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_unit0, R->ref_unit0.data(), n_ref * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_units, R->ref_units.data(), n_ref * sizeof(uint32_t), hipMemcpyHostToDevice, st));

    // ---- the file's pair table (bsig_types.h): the BSIG_PACK_CODES most frequent (flag, mapq) pairs among a
    // sample of the short reads, most frequent first, ties by key -- the same table on every GPU that lays
    // out the same columns.  env BAMSIGNALS_PACK=0: no packed class (testing; every short read in class 0).
    uint16_t *d_codemap = nullptr;
    if (!(getenv("BAMSIGNALS_PACK") && !strcmp(getenv("BAMSIGNALS_PACK"), "0"))) {
        constexpr uint32_t kKeys = 1u << 20, kPairCap = 16384;
        // one block for the counters, the pair list, its length and the code map: 4 MB + 128 KB + 2 MB
        uint8_t *blk;
        HIP_TRY(tmp.alloc(&blk, (size_t)kKeys * 4 + kPairCap * 8 + 256 + (size_t)kKeys * 2));
        uint32_t *d_hist = (uint32_t *)blk;
        uint2 *d_pairs = (uint2 *)(blk + (size_t)kKeys * 4);
        uint32_t *d_npairs = (uint32_t *)(blk + (size_t)kKeys * 4 + kPairCap * 8);
        d_codemap = (uint16_t *)(blk + (size_t)kKeys * 4 + kPairCap * 8 + 256);
        HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)kKeys * 4 + kPairCap * 8 + 256, st));
        HIP_TRY(hipMemsetAsync(d_codemap, 0xFF, (size_t)kKeys * 2, st));
        HIP_TRY(bsig::launch_pair_sample(n, d_pos, d_end, d_flag, d_mapq, d_hist, d_pairs, kPairCap, d_npairs, st));
        uint32_t n_pairs = 0;
        HIP_TRY(hipMemcpyAsync(&n_pairs, d_npairs, sizeof n_pairs, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<uint2> pairs;
        if (n_pairs <= kPairCap) {
            pairs.resize(n_pairs);
            if (n_pairs) HIP_TRY(hipMemcpyAsync(pairs.data(), d_pairs, (size_t)n_pairs * sizeof(uint2), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        } else {
            // more distinct pairs than the list holds (which of them it caught depends on timing): read the counters
            std::vector<uint32_t> hist(kKeys);
            HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, (size_t)kKeys * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (uint32_t k = 0; k < kKeys; ++k)
                if (hist[k]) pairs.push_back(make_uint2(k, hist[k]));
        }
        std::sort(pairs.begin(), pairs.end(), [](const uint2 &x, const uint2 &y) { return x.y != y.y ? x.y > y.y : x.x < y.x; });
        const int n_codes = (int)std::min<size_t>(pairs.size(), BSIG_PACK_CODES);
        if (n_codes > 0) {
            std::vector<uint32_t> fmtab(BSIG_PACK_CODES, 0u);
            for (int c = 0; c < n_codes; ++c) fmtab[(size_t)c] = (pairs[(size_t)c].x & 0xFFFu) | (pairs[(size_t)c].x >> 12) << 16;
            uint32_t *d_fmtab;
            HIP_TRY(R->pool.alloc(&d_fmtab, BSIG_PACK_CODES));
            HIP_TRY(hipMemcpyAsync(d_fmtab, fmtab.data(), BSIG_PACK_CODES * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(bsig::launch_codemap_fill(d_fmtab, n_codes, d_codemap, st));
            HIP_TRY(hipStreamSynchronize(st));          // (fmtab is a local)
            R->dev.fmtab = d_fmtab;
            R->dev.n_codes = n_codes;
            R->fmtab = fmtab;
        } else {
            d_codemap = nullptr;
        }
        if (diag) fprintf(stderr, "  [layout] pair table: %u pairs in the sample, %d codes, %.1f ms\n", n_pairs, n_codes, diag_ms());
    }

    // classes: per-chunk counts -> host exclusive scan
    const int64_t n_chunks = bsig::prep_chunks(n);
    uint32_t *d_counts;
    int32_t *d_maxspan;
    HIP_TRY(tmp.alloc(&d_counts, n_chunks * BSIG_MAX_CLASSES));
    HIP_TRY(tmp.alloc(&d_maxspan, BSIG_MAX_CLASSES + 1));
    HIP_TRY(hipMemsetAsync(d_maxspan, 0, (BSIG_MAX_CLASSES + 1) * sizeof(int32_t), st));
    HIP_TRY(bsig::launch_span_hist(n, n_ref, d_ref_off, d_units, d_pos, d_end, d_flag, d_mapq, d_codemap, d_counts, d_maxspan, st));
    // (the scan of the chunk counts stays on the device: only the class totals and the longest spans come back)
    uint64_t *d_base, *d_totals;
    HIP_TRY(tmp.alloc(&d_base, (size_t)n_chunks * BSIG_MAX_CLASSES));
    HIP_TRY(tmp.alloc(&d_totals, BSIG_MAX_CLASSES));
    HIP_TRY(bsig::launch_chunk_scan(n_chunks, d_counts, d_base, d_totals, st));
    int32_t maxspan[BSIG_MAX_CLASSES + 1];
    uint64_t class_n[BSIG_MAX_CLASSES] = {};
    HIP_TRY(hipMemcpyAsync(class_n, d_totals, sizeof class_n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(maxspan, d_maxspan, sizeof maxspan, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (maxspan[BSIG_MAX_CLASSES])
        return fail(BSIG_ERR_ARG, "reads must be sorted by position inside every reference (coordinate-sorted BAM order)");
    if (diag) fprintf(stderr, "  [layout] class counts %.1f ms\n", diag_ms());

    // bucket width per class: about 16 reads per bucket, 16 bp .. 64 kbp (the packed class: at most one
    // chunk of its position bits)
    bsig::ScatterPtrs S{};
    uint64_t n_buckets[BSIG_MAX_CLASSES] = {};
    int min_shift = 4;
    while ((total_bp >> min_shift) >= (1ull << 32)) ++min_shift;
    if (min_shift > BSIG_PACK_POS_BITS) return fail(BSIG_ERR_ARG, "genome too large for the bucket index");
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        BsigClassCols &C = R->dev.cls[c];
        C = BsigClassCols{};
        if (class_n[c] == 0) continue;
        if (class_n[c] >= (1ull << 32) - 8) return fail(BSIG_ERR_ARG, "more than 2^32 reads in one span class");
        double per_bucket = 16.0;
        if (const char *v = getenv("BAMSIGNALS_BUCKET_READS")) per_bucket = std::max(1.0, atof(v));
        const double bp_per_bucket = per_bucket * (double)total_bp / (double)class_n[c];
        const int max_shift = c == BSIG_CLASS_PACKED ? BSIG_PACK_POS_BITS : BSIG_REF_UNIT_SHIFT;
        int k = 4;
        while (k < max_shift && (double)(1ull << (k + 1)) <= bp_per_bucket) ++k;
        k = std::max(k, min_shift);
        if (k > max_shift) return fail(BSIG_ERR_ARG, "genome too large for the bucket index");
        const size_t cap = ((size_t)class_n[c] + 3) / 4 * 4 + 4;
        int32_t *p = nullptr, *e = nullptr, *t;
        uint32_t *f, *gb, *idx;
        if (c != BSIG_CLASS_PACKED) HIP_TRY(R->pool.alloc(&p, cap));      // a packed word carries its position
        if (c == 2 || c == 3) HIP_TRY(R->pool.alloc(&e, cap));           // classes 0, 1 and packed keep their span in fm
        HIP_TRY(R->pool.alloc(&f, cap));
        HIP_TRY(R->pool.alloc(&t, cap));
        HIP_TRY(tmp.alloc(&gb, cap));
        n_buckets[c] = total_bp >> k;
        HIP_TRY(R->pool.alloc(&idx, n_buckets[c] + 2));
        R->col_cap[c] = cap;
        R->idx_entries[c] = n_buckets[c] + 2;
        // the tail padding is read by the 16-B loads: keep it defined
        if (p) HIP_TRY(hipMemsetAsync(p + cap - 8, 0, 8 * sizeof(int32_t), st));
        if (e) HIP_TRY(hipMemsetAsync(e + cap - 8, 0, 8 * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(f + cap - 8, 0, 8 * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(t + cap - 8, 0, 8 * sizeof(int32_t), st));
        C.pos = p; C.end = e; C.fm = f; C.tlen = t; C.idx = idx;
        C.n = (int64_t)class_n[c]; C.maxspan = maxspan[c]; C.kshift = k;
        S.pos[c] = p; S.end[c] = e; S.fm[c] = f; S.tlen[c] = t; S.gb[c] = gb; S.kshift[c] = k;
        R->info.class_n[c] = C.n;
        R->info.class_maxspan[c] = C.maxspan;
        R->info.class_bucket_shift[c] = k;
        R->info.n_classes += 1;
    }
    R->info.n_codes = R->dev.n_codes;

    if (diag) fprintf(stderr, "  [layout] column + index allocations %.1f ms\n", diag_ms());
    HIP_TRY(bsig::launch_scatter(n, n_ref, d_ref_off, d_unit0, d_units, d_pos, d_end, d_flag, d_mapq, d_tlen, d_codemap,
                                 d_base, S, st));
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c)
        if (class_n[c])
            HIP_TRY(bsig::launch_build_idx((int64_t)class_n[c], S.gb[c], n_buckets[c],
                                           const_cast<uint32_t *>(R->dev.cls[c].idx), st));
    HIP_TRY(hipStreamSynchronize(st));
    if (diag) fprintf(stderr, "  [layout] scatter + indexes %.1f ms\n", diag_ms());
    R->info.hbm_bytes = R->pool.footprint();
    return make_packed_half(R, st);
}

int bsig::check_columns(const bsig_columns *cols)
{
    const int64_t n = cols->n_reads;
    if (n < 0 || cols->n_ref < 0) return fail(BSIG_ERR_ARG, "negative read or reference count");
    if (cols->n_ref > 0 && (!cols->ref_len || !cols->ref_off)) return fail(BSIG_ERR_ARG, "ref_len/ref_off missing");
    if (n > 0) {
        if (!cols->pos || !cols->flag || !cols->mapq || !cols->tlen) return fail(BSIG_ERR_ARG, "read columns missing");
        if (!cols->end && (!cols->cigar_off || !cols->cigar)) return fail(BSIG_ERR_ARG, "need either end or cigar_off+cigar");
        if (cols->n_ref == 0) return fail(BSIG_ERR_ARG, "reads without references");
    }
    if (cols->n_ref > 0) {
        if (cols->ref_off[0] != 0 || cols->ref_off[cols->n_ref] != n)
            return fail(BSIG_ERR_ARG, "ref_off must run from 0 to n_reads");
        for (int r = 0; r < cols->n_ref; ++r)
            if (cols->ref_off[r] > cols->ref_off[r + 1]) return fail(BSIG_ERR_ARG, "ref_off must be non-decreasing");
    }
    return BSIG_OK;
}

extern "C" {

static int upload_impl(bsig_ctx *ctx, const bsig_columns *cols, bsig_reads *R)
{
    const int64_t n = cols->n_reads;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    for (int r = 0; r < cols->n_ref; ++r)
        if (cols->ref_len[r] < 0) return fail(BSIG_ERR_ARG, "negative length of reference %d", r);
    if (n == 0 || cols->n_ref == 0)
        return bsig::layout_from_device(ctx, R, n, cols->n_ref, cols->ref_len, cols->ref_off, nullptr, nullptr, nullptr,
                                        nullptr, nullptr);
    DevPool tmp;
    int32_t *d_pos, *d_end, *d_tlen;
    uint16_t *d_flag;
    uint8_t *d_mapq;
    HIP_TRY(tmp.alloc(&d_pos, n));
    HIP_TRY(tmp.alloc(&d_end, n));
    HIP_TRY(tmp.alloc(&d_tlen, n));
    HIP_TRY(tmp.alloc(&d_flag, n));
    HIP_TRY(tmp.alloc(&d_mapq, n));
    HIP_TRY(hipMemcpyAsync(d_pos, cols->pos, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tlen, cols->tlen, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_flag, cols->flag, n * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_mapq, cols->mapq, n * sizeof(uint8_t), hipMemcpyHostToDevice, st));
    if (cols->end) {
        HIP_TRY(hipMemcpyAsync(d_end, cols->end, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    } else {
        const int64_t n_ops = cols->cigar_off[n];
        if (cols->cigar_off[0] != 0 || n_ops < 0) return fail(BSIG_ERR_ARG, "cigar_off must start at 0 and be non-decreasing");
        int64_t *d_coff;
        uint32_t *d_cig;
        HIP_TRY(tmp.alloc(&d_coff, n + 1));
        HIP_TRY(tmp.alloc(&d_cig, n_ops));
        HIP_TRY(hipMemcpyAsync(d_coff, cols->cigar_off, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (n_ops) HIP_TRY(hipMemcpyAsync(d_cig, cols->cigar, n_ops * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(bsig::launch_cigar_end(n, d_pos, d_flag, d_coff, d_cig, d_end, st));
    }
    // layout_from_device synchronises the stream before it returns: tmp may be released then
    return bsig::layout_from_device(ctx, R, n, cols->n_ref, cols->ref_len, cols->ref_off, d_pos, d_end, d_flag, d_mapq,
                                    d_tlen);
}

int bsig_reads_upload(bsig_ctx *ctx, const bsig_columns *cols, bsig_reads **out)
{
    if (!ctx || !cols || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_reads_upload");
    *out = nullptr;
    if (const int rc = bsig::check_columns(cols)) return rc;
    bsig_reads *R = new bsig_reads;
    R->ctx = ctx;
    const int rc = upload_impl(ctx, cols, R);
    if (rc != BSIG_OK) { delete R; return rc; }
    *out = R;
    return BSIG_OK;
}

int bsig_reads_get_info(const bsig_reads *reads, bsig_reads_info *info)
{
    if (!reads || !info) return fail(BSIG_ERR_ARG, "NULL argument");
    *info = reads->info;
    return BSIG_OK;
}

void bsig_reads_free(bsig_reads *reads) { delete reads; }

int bsig_reads_clone(const bsig_reads *src, bsig_ctx *dst_ctx, bsig_reads **out)
{
    if (!src || !dst_ctx || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_reads_clone");
    *out = nullptr;
    const int sdev = src->ctx->device, ddev = dst_ctx->device;
    HIP_TRY(hipSetDevice(ddev));
    if (sdev != ddev) {
        // direct copies over xGMI where the link allows it; without peer access the runtime stages
        // the copy through the host, which is still correct
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, ddev, sdev) == hipSuccess && can) {
            (void)hipDeviceEnablePeerAccess(sdev, 0);     // "already enabled" is fine
            (void)hipGetLastError();
        }
    }
    bsig_reads *R = new bsig_reads;
    R->ctx = dst_ctx;
    // a layout of its own: with the 0 a new set starts with, a plan's second run on the clone took its windows for looked
    // up already (resolved_gen 0 == layout_gen 0, run_main) and read a table nothing had written
    R->layout_gen = bsig::next_layout_gen();
    R->info = src->info;
    R->spliced = src->spliced;
    R->n_ref = src->n_ref;
    R->ref_unit0 = src->ref_unit0;
    R->ref_units = src->ref_units;
    R->ref_len = src->ref_len;
    R->fmtab = src->fmtab;
    R->dev.fmtab = nullptr;
    R->dev.n_codes = src->dev.n_codes;
    hipStream_t st = dst_ctx->stream;
    hipError_t e = hipSuccess;
    auto copy = [&](const void *from, size_t bytes, void **to) {
        if (e != hipSuccess || !from) { *to = nullptr; return; }
        uint8_t *q = nullptr;
        e = R->pool.alloc(&q, bytes);
        if (e == hipSuccess) e = hipMemcpyPeerAsync(q, ddev, from, sdev, bytes, st);
        *to = q;
    };
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        const BsigClassCols &S = src->dev.cls[c];
        BsigClassCols &D = R->dev.cls[c];
        D = S;
        if (S.n == 0) continue;
        R->col_cap[c] = src->col_cap[c];
        R->idx_entries[c] = src->idx_entries[c];
        const size_t cb = (size_t)src->col_cap[c] * sizeof(int32_t);
        void *p;
        copy(S.pos, cb, &p); D.pos = (const int32_t *)p;
        copy(S.end, cb, &p); D.end = (const int32_t *)p;
        copy(S.fm, cb, &p); D.fm = (const uint32_t *)p;
        copy(S.tlen, cb, &p); D.tlen = (const int32_t *)p;
        copy(S.idx, (size_t)src->idx_entries[c] * sizeof(uint32_t), &p); D.idx = (const uint32_t *)p;
    }
    {
        void *p;
        copy(src->dev.fmtab, BSIG_PACK_CODES * sizeof(uint32_t), &p);
        R->dev.fmtab = (const uint32_t *)p;
    }
    if (src->junc.n > 0) {      // a spliced set's junction table (junctions.hip)
        const bsig_reads::Junctions &S = src->junc;
        bsig_reads::Junctions &D = R->junc;
        const size_t rows = (size_t)S.n;
        void *p;
        copy(S.start, rows * sizeof(int32_t), &p); D.start = (const int32_t *)p;
        copy(S.end, rows * sizeof(int32_t), &p); D.end = (const int32_t *)p;
        copy(S.fm, rows * sizeof(uint32_t), &p); D.fm = (const uint32_t *)p;
        copy(S.anchor, rows * sizeof(int32_t), &p); D.anchor = (const int32_t *)p;
        copy(S.ref_off, ((size_t)src->n_ref + 1) * sizeof(int64_t), &p); D.ref_off = (const int64_t *)p;
        D.n = S.n;
    }
    R->junc.h_ref_off = src->junc.h_ref_off;
    if (src->rtab.n > 0) {      // a spliced set's read table (splice.hip, genecounts.hip)
        const bsig_reads::ReadTable &S = src->rtab;
        bsig_reads::ReadTable &D = R->rtab;
        const size_t reads = (size_t)S.n, blocks = (size_t)std::max<int64_t>(S.n_blocks, 1);
        void *p;
        copy(S.blk_off, (reads + 1) * sizeof(uint32_t), &p); D.blk_off = (const uint32_t *)p;
        copy(S.fm, reads * sizeof(uint32_t), &p); D.fm = (const uint32_t *)p;
        copy(S.bstart, blocks * sizeof(int32_t), &p); D.bstart = (const int32_t *)p;
        copy(S.bend, blocks * sizeof(int32_t), &p); D.bend = (const int32_t *)p;
        copy(S.ref_off, ((size_t)src->n_ref + 1) * sizeof(int64_t), &p); D.ref_off = (const int64_t *)p;
        D.n = S.n;
        D.n_blocks = S.n_blocks;
    }
    R->rtab.h_ref_off = src->rtab.h_ref_off;
    if (src->btab.present && src->btab.n > 0) {     // a set with bases: its base table (nucleotides.hip)
        const bsig_reads::BaseTable &S = src->btab;
        bsig_reads::BaseTable &D = R->btab;
        const size_t reads = (size_t)S.n;
        void *p;
        copy(S.pos, reads * sizeof(int32_t), &p); D.pos = (const int32_t *)p;
        copy(S.endmax, reads * sizeof(int32_t), &p); D.endmax = (const int32_t *)p;
        copy(S.fm, reads * sizeof(uint32_t), &p); D.fm = (const uint32_t *)p;
        copy(S.cig_off, (reads + 1) * sizeof(int64_t), &p); D.cig_off = (const int64_t *)p;
        copy(S.seq_off, (reads + 1) * sizeof(int64_t), &p); D.seq_off = (const int64_t *)p;
        copy(S.cigar, (size_t)std::max<int64_t>(S.n_ops, 1) * sizeof(uint32_t), &p); D.cigar = (const uint32_t *)p;
        copy(S.seq, (size_t)std::max<int64_t>((S.n_bases + 1) / 2, 1), &p); D.seq = (const uint8_t *)p;
        copy(S.qual, (size_t)std::max<int64_t>(S.n_bases, 1), &p); D.qual = (const uint8_t *)p;
        copy(S.ref_off, ((size_t)src->n_ref + 1) * sizeof(int64_t), &p); D.ref_off = (const int64_t *)p;
        D.n = S.n; D.n_ops = S.n_ops; D.n_bases = S.n_bases;
    }
    R->btab.present = src->btab.present;
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        delete R;
        return fail(e == hipErrorOutOfMemory ? BSIG_ERR_NOMEM : BSIG_ERR_DEVICE, "copying the reads to GPU %d failed: %s", ddev,
                    hipGetErrorString(e));
    }
    R->info.hbm_bytes = R->pool.footprint();
    // (D = S above took the source's p5h: the clone makes its own, under this process's BAMSIGNALS_PACKED_HALF)
    if (const int rc = make_packed_half(R, st)) {
        delete R;
        return rc;
    }
    *out = R;
    return BSIG_OK;
}

}  // extern "C"

namespace {

// Result download into PAGEABLE host memory (an R vector, a numpy array): the runtime's own
// pageable path stages through one buffer and is first-touch bound on the destination pages
// (80 MB in 8 ms).  Here the result crosses PCIe by DMA into two page-locked halves and a few
// threads move each half on into the destination while the next one is in flight.
struct DownloadStage {
    std::mutex mu;
    hipEvent_t ev[2] = {nullptr, nullptr};
    static constexpr size_t kHalf = 32u << 20;          // (the halves are the device's PinnedPair)
    int ensure()
    {
        for (int k = 0; k < 2; ++k)
            if (!ev[k]) HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        return BSIG_OK;
    }
};
// one per GPU: the events belong to the device they were created on
DownloadStage &download_for(int device)
{
    static std::mutex mu;
    static std::vector<std::pair<int, DownloadStage *>> all;
    std::lock_guard<std::mutex> lk(mu);
    for (auto &kv : all)
        if (kv.first == device) return *kv.second;
    all.emplace_back(device, new DownloadStage);
    return *all.back().second;
}

}  // namespace
int bsig::PinnedPair::ensure(size_t bytes)
{
    if (cap >= bytes) return BSIG_OK;
    for (int k = 0; k < 2; ++k) {
        if (buf[k]) (void)bsig::metered_host_free(buf[k]);
        buf[k] = nullptr;
    }
    cap = 0;
    for (int k = 0; k < 2; ++k) HIP_TRY(bsig::metered_host_malloc((void **)&buf[k], bytes));
    cap = bytes;
    return BSIG_OK;
}
bsig::PinnedPair &bsig::pinned_pair_for(int device)
{
    static std::mutex mu;
    static std::vector<std::pair<int, PinnedPair *>> all;
    std::lock_guard<std::mutex> lk(mu);
    for (auto &kv : all)
        if (kv.first == device) return *kv.second;
    all.emplace_back(device, new PinnedPair);
    return *all.back().second;
}
namespace {
bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// One or more slices of device memory to host memory through the two page-locked halves: the slices are laid
// back to back into chunks of one half each (several DMA copies per chunk where slices are short), and while one
// half crosses PCIe a few threads move the other on -- sink(first cell of the flat result, source, cells) is
// called by several threads at once, on disjoint pieces.
struct DlSlice { const uint8_t *src; size_t bytes; int64_t dst_c0; };      // bytes: a multiple of 4
typedef std::function<void(int64_t, const int32_t *, int64_t)> DownloadSink;
int download_staged(int device, hipStream_t st, const std::vector<DlSlice> &slices, const DownloadSink &sink, int copy_threads = 0)
{
    DownloadStage &g_download = download_for(device);
    std::lock_guard<std::mutex> lock(g_download.mu);
    HIP_TRY(hipSetDevice(device));
    int rc = g_download.ensure();
    if (rc) return rc;
    bsig::PinnedPair &pair = bsig::pinned_pair_for(device);
    std::lock_guard<std::mutex> pair_lock(pair.mu);
    rc = pair.ensure(DownloadStage::kHalf);
    if (rc) return rc;
    const size_t half = DownloadStage::kHalf;
    struct Part { size_t at; const uint8_t *src; size_t len; int64_t dst_c0; };      // `at`: offset in the half
    struct Chunk { size_t p0, p1, len; };                                              // parts [p0, p1)
    std::vector<Part> parts;
    std::vector<Chunk> chunks;
    {
        size_t fill = 0, first = 0;
        for (const DlSlice &sl : slices) {
            size_t done_b = 0;
            while (done_b < sl.bytes) {
                if (fill == half) { chunks.push_back(Chunk{first, parts.size(), fill}); first = parts.size(); fill = 0; }
                const size_t take = std::min(sl.bytes - done_b, half - fill);
                parts.push_back(Part{fill, sl.src + done_b, take, sl.dst_c0 + (int64_t)(done_b / 4)});
                fill += take;
                done_b += take;
            }
        }
        if (fill) chunks.push_back(Chunk{first, parts.size(), fill});
    }
    const size_t n_chunks = chunks.size();
    if (n_chunks == 0) return BSIG_OK;
    int n_thr = 8;
    if (const char *e = getenv("BAMSIGNALS_COPY_THREADS")) n_thr = std::max(1, std::min(64, atoi(e)));
    if (copy_threads > 0) n_thr = copy_threads;
    std::atomic<int64_t> ready(-1);                 // chunks 0..ready are in their half
    std::vector<std::atomic<int>> done(n_chunks);   // workers finished with chunk c
    for (auto &d : done) d.store(0);
    std::atomic<bool> abort(false);
    // thread t's share of chunk c: bytes [len * t / n, len * (t + 1) / n) of the half, cut at 4-byte cells
    auto share = [&](size_t c, int t) {
        const Chunk &C = chunks[c];
        const size_t a = (C.len * (size_t)t / (size_t)n_thr) & ~(size_t)3;
        const size_t b = t + 1 == n_thr ? C.len : (C.len * (size_t)(t + 1) / (size_t)n_thr) & ~(size_t)3;
        const uint8_t *buf = pair.buf[c & 1];
        for (size_t p = C.p0; p < C.p1 && a < b; ++p) {
            const Part &P = parts[p];
            const size_t lo = std::max(a, P.at), hi = std::min(b, P.at + P.len);
            if (lo < hi) sink(P.dst_c0 + (int64_t)((lo - P.at) / 4), (const int32_t *)(buf + lo), (int64_t)((hi - lo) / 4));
        }
    };
    auto worker = [&](int t) {
        for (size_t c = 0; c < n_chunks; ++c) {
            while (ready.load(std::memory_order_acquire) < (int64_t)c) {
                if (abort.load()) return;
                std::this_thread::yield();
            }
            share(c, t);
            done[c].fetch_add(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < n_thr; ++t) th.emplace_back(worker, t);
    hipError_t e = hipSuccess;
    auto issue = [&](size_t c) {
        const Chunk &C = chunks[c];
        for (size_t p = C.p0; p < C.p1 && e == hipSuccess; ++p)
            e = hipMemcpyAsync(pair.buf[c & 1] + parts[p].at, parts[p].src, parts[p].len, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(g_download.ev[c & 1], st);
    };
    for (size_t c = 0; c < std::min<size_t>(2, n_chunks) && e == hipSuccess; ++c) issue(c);
    for (size_t c = 0; c < n_chunks && e == hipSuccess; ++c) {
        e = hipEventSynchronize(g_download.ev[c & 1]);
        if (e != hipSuccess) break;
        ready.store((int64_t)c, std::memory_order_release);
        share(c, 0);                              // the calling thread is worker 0 of this chunk
        done[c].fetch_add(1, std::memory_order_release);
        while (done[c].load(std::memory_order_acquire) < n_thr) std::this_thread::yield();
        if (c + 2 < n_chunks) issue(c + 2);       // this half is free again
    }
    if (e != hipSuccess) abort.store(true);
    ready.store((int64_t)n_chunks, std::memory_order_release);
    for (auto &t : th) t.join();
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(BSIG_ERR_DEVICE, "result download failed: %s", hipGetErrorString(e));
    }
    return BSIG_OK;
}

}  // namespace

int bsig::download_to_host(bsig_ctx *ctx, const void *src_dev, void *dst_host, size_t bytes)
{
    if (bytes == 0) return BSIG_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (bytes >= (8u << 20) && !is_pinned_host(dst_host) && bytes % 4 == 0) {
        int32_t *dst = (int32_t *)dst_host;
        return download_staged(ctx->device, ctx->stream, {DlSlice{(const uint8_t *)src_dev, bytes, 0}},
                               [dst](int64_t c0, const int32_t *src, int64_t cells) { memcpy(dst + c0, src, (size_t)cells * 4); });
    }
    hipError_t e = hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(BSIG_ERR_DEVICE, "result download failed: %s", hipGetErrorString(e));
    return BSIG_OK;
}

void bsig::HostDest::put(int64_t c0, const int32_t *src, int64_t count) const
{
    if (count <= 0) return;
    if (flat) { memcpy(flat + c0, src, (size_t)count * sizeof(int32_t)); return; }
    // the range that holds cell c0: the last i with off[i] <= c0 (empty ranges in between are skipped by the loop)
    int64_t i = (int64_t)(std::upper_bound(off, off + n + 1, c0) - off) - 1;
    while (count > 0 && i < n) {
        const int64_t end = off[i + 1];
        if (end <= c0) { ++i; continue; }
        const int64_t take = std::min(count, end - c0);
        memcpy(ptrs[i] + (c0 - off[i]), src, (size_t)take * sizeof(int32_t));
        c0 += take; src += take; count -= take;
        ++i;
    }
}

// The result straight into its final place: into one flat buffer, or range by range into the vectors the
// caller made for them (no flat staging copy of the result in host memory: the reference counts into the R
// vectors themselves, ref: src/bamsignals.cpp:172-190,361-362).  Large results cross PCIe by DMA into two
// page-locked halves, and a few threads move each half on -- range by range where the destination is one.
int bsig::download_to_dest(bsig_ctx *ctx, const int32_t *src_dev, const HostDest &dst, int64_t cells)
{
    return download_slice_to_dest(ctx, src_dev, dst, 0, cells, 0);
}

int bsig::download_slices_to_dest(bsig_ctx *ctx, const int32_t *src_dev, int64_t n_slices, const int64_t *src_c0, const int64_t *dst_c0,
                                  const int64_t *cells, const HostDest &dst, int copy_threads)
{
    std::vector<DlSlice> sl;
    int64_t total = 0;
    for (int64_t k = 0; k < n_slices; ++k)
        if (cells[k] > 0) { sl.push_back(DlSlice{(const uint8_t *)(src_dev + src_c0[k]), (size_t)cells[k] * 4, dst_c0[k]}); total += cells[k]; }
    if (sl.empty()) return BSIG_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (dst.flat && sl.size() == 1 && copy_threads == 0) return download_to_host(ctx, sl[0].src, dst.flat + sl[0].dst_c0, sl[0].bytes);
    if ((size_t)total * 4 < (1u << 20)) {
        // a small result: through a buffer of its own (the runtime stages a copy into pageable memory anyway)
        std::vector<int32_t> tmp((size_t)total);
        hipError_t e = hipSuccess;
        int64_t at = 0;
        for (const DlSlice &q : sl) {
            if (e == hipSuccess) e = hipMemcpyAsync(tmp.data() + at, q.src, q.bytes, hipMemcpyDeviceToHost, ctx->stream);
            at += (int64_t)(q.bytes / 4);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(BSIG_ERR_DEVICE, "result download failed: %s", hipGetErrorString(e));
        at = 0;
        for (const DlSlice &q : sl) { dst.put(q.dst_c0, tmp.data() + at, (int64_t)(q.bytes / 4)); at += (int64_t)(q.bytes / 4); }
        return BSIG_OK;
    }
    const HostDest *D = &dst;
    return download_staged(ctx->device, ctx->stream, sl, [D](int64_t c0, const int32_t *src, int64_t n) { D->put(c0, src, n); }, copy_threads);
}

int bsig::download_slice_to_dest(bsig_ctx *ctx, const int32_t *src_dev, const HostDest &dst, int64_t c0, int64_t cells, int copy_threads)
{
    const int64_t zero = 0;
    return download_slices_to_dest(ctx, src_dev, 1, &zero, &c0, &cells, dst, copy_threads);
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// the resident layout as a file (the decoded-column sidecar of SURVEY 8f.4)
// ---------------------------------------------------------------------------------------------
namespace {
struct SidecarClass {
    int64_t n;
    int32_t maxspan, kshift;
    uint64_t col_cap, idx_entries;
};
struct SidecarHeader {
    char magic[8];                  // "BSIGRDS1"
    uint32_t version, n_ref;
    int64_t n_reads;
    uint32_t stamp_len, n_classes;
    uint64_t file_bytes;
    SidecarClass cls[BSIG_MAX_CLASSES];
    uint64_t checksum;              // of every column, index and the pair table as they lay in HBM when the file was written
    uint32_t n_codes, reserved;     // pairs in the packed class's table (the table follows the reference arrays)
};
constexpr uint32_t kSidecarVersion = 4;
// which columns a class has: pos (all but the packed class), end (classes 2 and 3), fm, tlen
inline bool class_has_pos(int c) { return c != BSIG_CLASS_PACKED; }
inline bool class_has_end(int c) { return c == 2 || c == 3; }
inline int class_columns(int c) { return 2 + (class_has_pos(c) ? 1 : 0) + (class_has_end(c) ? 1 : 0); }
inline uint64_t pad64(uint64_t v) { return (v + 63) & ~(uint64_t)63; }
}  // namespace

namespace {
// checksum of the class columns and indexes of a resident layout, computed where they lie (kernels.hip)
int layout_checksum(const bsig_reads *R, uint64_t *out)
{
    hipStream_t st = R->ctx->stream;
    HIP_TRY(hipSetDevice(R->ctx->device));
    unsigned long long *d_acc = nullptr, acc = 0;
    HIP_TRY(hipMalloc((void **)&d_acc, sizeof acc));
    hipError_t e = hipMemsetAsync(d_acc, 0, sizeof acc, st);
    uint64_t salt = 1;
    for (int c = 0; c < BSIG_MAX_CLASSES && e == hipSuccess; ++c) {
        const BsigClassCols &C = R->dev.cls[c];
        if (!C.n) continue;
        const uint64_t cap = R->col_cap[c];
        for (const void *col : {(const void *)C.pos, (const void *)C.end, (const void *)C.fm, (const void *)C.tlen}) {
            if (col && e == hipSuccess) e = bsig::launch_checksum(col, cap, salt, d_acc, st);
            salt += 0x100000001ull;
        }
        // (the index's spare last entry is never written: not part of the sum)
        if (e == hipSuccess) e = bsig::launch_checksum(C.idx, R->idx_entries[c] - 1, salt, d_acc, st);
        salt += 0x100000001ull;
    }
    if (R->dev.fmtab && e == hipSuccess) e = bsig::launch_checksum(R->dev.fmtab, BSIG_PACK_CODES, salt, d_acc, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_acc);
    if (e != hipSuccess) return fail(BSIG_ERR_DEVICE, "layout checksum failed: %s", hipGetErrorString(e));
    *out = (uint64_t)acc;
    return BSIG_OK;
}
}  // namespace

int bsig_reads_save(const bsig_reads *reads, const char *path, const char *stamp)
{
    if (!reads || !path || !stamp) return fail(BSIG_ERR_ARG, "NULL argument to bsig_reads_save");
    if (reads->spliced)
        return fail(BSIG_ERR_ARG, "spliced reads have no reads file: the format has no mark for rows that are aligned blocks, and a "
                                  "loader would take them for reads");
    if (reads->btab.present)
        return fail(BSIG_ERR_ARG, "reads with bases have no reads file: the format holds no base table, and a loader would "
                                  "give back a set without one");
    HIP_TRY(hipSetDevice(reads->ctx->device));
    SidecarHeader H;
    memset(&H, 0, sizeof H);
    memcpy(H.magic, "BSIGRDS1", 8);
    H.version = kSidecarVersion;
    H.n_ref = (uint32_t)reads->n_ref;
    H.n_reads = reads->info.n_reads;
    H.stamp_len = (uint32_t)strlen(stamp);
    H.n_classes = (uint32_t)reads->info.n_classes;
    H.n_codes = (uint32_t)reads->dev.n_codes;
    uint64_t bytes = pad64(sizeof H) + pad64(H.stamp_len) + 3 * pad64((uint64_t)H.n_ref * 4) + (H.n_codes ? pad64(BSIG_PACK_CODES * 4) : 0);
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        const BsigClassCols &C = reads->dev.cls[c];
        H.cls[c] = SidecarClass{C.n, C.maxspan, C.kshift, C.n ? reads->col_cap[c] : 0, C.n ? reads->idx_entries[c] : 0};
        if (!C.n) continue;
        bytes += class_columns(c) * pad64(H.cls[c].col_cap * 4) + pad64(H.cls[c].idx_entries * 4);
    }
    H.file_bytes = bytes;
    {
        const int crc_rc = layout_checksum(reads, &H.checksum);
        if (crc_rc) return crc_rc;
    }
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long long)getpid());
    FILE *fp = fopen(tmp.c_str(), "wb");
    if (!fp) return fail(BSIG_ERR_IO, "cannot write %s", tmp.c_str());
    bool ok = true;
    static const char zeros[64] = {0};
    auto put = [&](const void *p, uint64_t n) {
        ok = ok && (n == 0 || fwrite(p, 1, n, fp) == n);
        const uint64_t pad = pad64(n) - n;
        ok = ok && (pad == 0 || fwrite(zeros, 1, pad, fp) == pad);
    };
    put(&H, sizeof H);
    put(stamp, H.stamp_len);
    put(reads->ref_len.data(), (uint64_t)H.n_ref * 4);
    put(reads->ref_unit0.data(), (uint64_t)H.n_ref * 4);
    put(reads->ref_units.data(), (uint64_t)H.n_ref * 4);
    if (H.n_codes) put(reads->fmtab.data(), BSIG_PACK_CODES * 4);
    std::vector<uint8_t> host;
    int rc = BSIG_OK;
    auto put_dev = [&](const void *d, uint64_t n) {
        if (rc || !ok) return;
        host.resize(n);
        rc = bsig::download_to_host(reads->ctx, d, host.data(), n);
        if (!rc) put(host.data(), n);
    };
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        const BsigClassCols &C = reads->dev.cls[c];
        if (!C.n) continue;
        if (class_has_pos(c)) put_dev(C.pos, H.cls[c].col_cap * 4);
        if (class_has_end(c)) put_dev(C.end, H.cls[c].col_cap * 4);
        put_dev(C.fm, H.cls[c].col_cap * 4);
        put_dev(C.tlen, H.cls[c].col_cap * 4);
        put_dev(C.idx, H.cls[c].idx_entries * 4);
    }
    ok = (fclose(fp) == 0) && ok;
    if (rc || !ok || rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        return rc ? rc : fail(BSIG_ERR_IO, "writing %s failed", path);
    }
    return BSIG_OK;
}

namespace {
// pageable host memory -> device through two page-locked halves filled by a few threads (the
// mirror image of download_staged)
int upload_staged(int device, hipStream_t st, const uint8_t *src, uint8_t *dst_dev, size_t bytes)
{
    DownloadStage &D = download_for(device);
    std::lock_guard<std::mutex> lock(D.mu);
    HIP_TRY(hipSetDevice(device));
    int rc = D.ensure();
    if (rc) return rc;
    bsig::PinnedPair &pair = bsig::pinned_pair_for(device);
    std::lock_guard<std::mutex> pair_lock(pair.mu);
    rc = pair.ensure(DownloadStage::kHalf);
    if (rc) return rc;
    const size_t half = DownloadStage::kHalf;
    int n_thr = 8;
    if (const char *e = getenv("BAMSIGNALS_COPY_THREADS")) n_thr = std::max(1, std::min(64, atoi(e)));
    bool used[2] = {false, false};
    size_t c = 0;
    for (size_t at = 0; at < bytes; at += half, ++c) {
        const size_t len = std::min(half, bytes - at);
        const int h = (int)(c & 1);
        if (used[h]) HIP_TRY(hipEventSynchronize(D.ev[h]));
        std::vector<std::thread> th;
        auto part = [&](int t) {
            const size_t a = len * (size_t)t / (size_t)n_thr, b = len * (size_t)(t + 1) / (size_t)n_thr;
            if (b > a) memcpy(pair.buf[h] + a, src + at + a, b - a);
        };
        for (int t = 1; t < n_thr; ++t) th.emplace_back(part, t);
        part(0);
        for (auto &x : th) x.join();
        HIP_TRY(hipMemcpyAsync(dst_dev + at, pair.buf[h], len, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(D.ev[h], st));
        used[h] = true;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return BSIG_OK;
}
}  // namespace

int bsig_reads_load(bsig_ctx *ctx, const char *path, const char *stamp, bsig_reads **out)
{
    if (!ctx || !path || !stamp || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_reads_load");
    *out = nullptr;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(BSIG_ERR_IO, "cannot open %s", path);
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (size_t)sb.st_size < sizeof(SidecarHeader)) { close(fd); return fail(BSIG_ERR_FORMAT, "%s is not a reads file", path); }
    const size_t size = (size_t)sb.st_size;
    void *map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (map == MAP_FAILED) return fail(BSIG_ERR_IO, "cannot map %s", path);
    const uint8_t *base = (const uint8_t *)map;
    struct Unmap { void *p; size_t n; ~Unmap() { munmap(p, n); } } unmap{map, size};
    SidecarHeader H;
    memcpy(&H, base, sizeof H);
    if (memcmp(H.magic, "BSIGRDS1", 8) != 0 || H.version != kSidecarVersion || H.file_bytes != size)
        return fail(BSIG_ERR_FORMAT, "%s is not a reads file of this version (or is truncated)", path);
    uint64_t at = pad64(sizeof H);
    auto take = [&](uint64_t n) -> const uint8_t * {
        if (at + pad64(n) > size) return nullptr;
        const uint8_t *p = base + at;
        at += pad64(n);
        return p;
    };
    const uint8_t *st_p = take(H.stamp_len);
    if (!st_p || H.stamp_len != strlen(stamp) || memcmp(st_p, stamp, H.stamp_len) != 0)
        return fail(BSIG_ERR_FORMAT, "%s was made from another version of the BAM file", path);
    if (H.n_ref > (1u << 28)) return fail(BSIG_ERR_FORMAT, "%s is damaged", path);
    const uint8_t *p_len = take((uint64_t)H.n_ref * 4), *p_u0 = take((uint64_t)H.n_ref * 4), *p_un = take((uint64_t)H.n_ref * 4);
    if (!p_len || !p_u0 || !p_un) return fail(BSIG_ERR_FORMAT, "%s is truncated", path);
    std::unique_ptr<bsig_reads> R(new bsig_reads);
    R->ctx = ctx;
    R->n_ref = (int32_t)H.n_ref;
    R->ref_len.assign((const int32_t *)p_len, (const int32_t *)p_len + H.n_ref);
    R->ref_unit0.assign((const uint32_t *)p_u0, (const uint32_t *)p_u0 + H.n_ref);
    R->ref_units.assign((const uint32_t *)p_un, (const uint32_t *)p_un + H.n_ref);
    R->info = bsig_reads_info{};
    R->info.n_reads = H.n_reads;
    R->layout_gen = bsig::next_layout_gen();
    // no table, no packed reads; the converse does not hold: the pair sample may have seen short reads of which
    // none qualified for the packed class (all beyond their reference's end), and such a layout is saved as it is
    if (H.n_codes > BSIG_PACK_CODES || (H.n_codes == 0 && H.cls[BSIG_CLASS_PACKED].n != 0))
        return fail(BSIG_ERR_FORMAT, "%s is damaged (pair table)", path);
    if (H.n_codes) {
        const uint8_t *p_tab = take(BSIG_PACK_CODES * 4);
        if (!p_tab) return fail(BSIG_ERR_FORMAT, "%s is truncated", path);
        R->fmtab.assign((const uint32_t *)p_tab, (const uint32_t *)p_tab + BSIG_PACK_CODES);
        // a code's pair: 12 flag bits, an 8-bit mapq, nothing else; unused entries zero
        for (uint32_t c = 0; c < BSIG_PACK_CODES; ++c)
            if ((R->fmtab[c] & 0xFF00F000u) || (c >= H.n_codes && R->fmtab[c]))
                return fail(BSIG_ERR_FORMAT, "%s is damaged (pair table)", path);
    }
    // The file's numbers steer device-side indexing (bucket numbers, read windows), so nothing is taken on
    // trust: the unit tables must be the ones layout_from_device derives from the reference lengths, every
    // class's shapes must follow from its read count and bucket shift, the counts must add up -- and below
    // the indexes are checked on the device and the checksum of what reached HBM must match the header's.
    uint64_t total_units = 0;
    for (uint32_t r = 0; r < H.n_ref; ++r) {
        if (R->ref_len[r] < 0) return fail(BSIG_ERR_FORMAT, "%s is damaged (reference lengths)", path);
        const uint64_t u = ((uint64_t)R->ref_len[r] >> BSIG_REF_UNIT_SHIFT) + 1;
        if (R->ref_unit0[r] != total_units || R->ref_units[r] != u || total_units + u >= (1ull << 31))
            return fail(BSIG_ERR_FORMAT, "%s is damaged (reference units)", path);
        total_units += u;
    }
    const uint64_t total_bp = total_units << BSIG_REF_UNIT_SHIFT;
    {
        int64_t sum = 0;
        uint32_t live = 0;
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
            if (H.cls[c].n < 0 || H.cls[c].n > H.n_reads) return fail(BSIG_ERR_FORMAT, "%s is damaged (class counts)", path);
            sum += H.cls[c].n;
            live += H.cls[c].n > 0;
        }
        if (H.n_reads < 0 || sum != H.n_reads || live != H.n_classes || (H.n_reads > 0 && H.n_ref == 0))
            return fail(BSIG_ERR_FORMAT, "%s is damaged (class counts)", path);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        BsigClassCols &C = R->dev.cls[c];
        C = BsigClassCols{};
        const SidecarClass &K = H.cls[c];
        if (K.n <= 0) continue;
        if ((uint64_t)K.n >= (1ull << 32) - 8 || K.col_cap != ((uint64_t)K.n + 3) / 4 * 4 + 4 || K.kshift < 4 ||
            K.kshift > (c == BSIG_CLASS_PACKED ? BSIG_PACK_POS_BITS : BSIG_REF_UNIT_SHIFT) || (c == BSIG_CLASS_PACKED && K.maxspan > 256) || (total_bp >> K.kshift) >= (1ull << 32) || K.idx_entries != (total_bp >> K.kshift) + 2 ||
            K.maxspan < 1)
            return fail(BSIG_ERR_FORMAT, "%s is damaged (shape of span class %d)", path, c);
        auto load = [&](uint64_t count, const void **dst) -> int {
            const uint8_t *src = take(count * 4);
            if (!src) return fail(BSIG_ERR_FORMAT, "%s is truncated", path);
            uint32_t *d = nullptr;
            HIP_TRY(R->pool.alloc(&d, (size_t)count));
            *dst = d;
            return upload_staged(ctx->device, ctx->stream, src, (uint8_t *)d, (size_t)count * 4);
        };
        int rc = BSIG_OK;
        if (class_has_pos(c)) rc = load(K.col_cap, (const void **)&C.pos);
        if (!rc && class_has_end(c)) rc = load(K.col_cap, (const void **)&C.end);
        if (!rc) rc = load(K.col_cap, (const void **)&C.fm);
        if (!rc) rc = load(K.col_cap, (const void **)&C.tlen);
        if (!rc) rc = load(K.idx_entries, (const void **)&C.idx);
        if (rc) return rc;
        C.n = K.n; C.maxspan = K.maxspan; C.kshift = K.kshift;
        R->col_cap[c] = K.col_cap;
        R->idx_entries[c] = K.idx_entries;
        R->info.class_n[c] = K.n;
        R->info.class_maxspan[c] = K.maxspan;
        R->info.class_bucket_shift[c] = K.kshift;
        R->info.n_classes += 1;
    }
    R->dev.fmtab = nullptr;
    R->dev.n_codes = (int32_t)H.n_codes;
    R->info.n_codes = (int32_t)H.n_codes;
    if (H.n_codes) {
        uint32_t *d = nullptr;
        HIP_TRY(R->pool.alloc(&d, BSIG_PACK_CODES));
        HIP_TRY(hipMemcpyAsync(d, R->fmtab.data(), BSIG_PACK_CODES * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        R->dev.fmtab = d;
    }
    R->info.hbm_bytes = R->pool.footprint();
    // what arrived in HBM: indexes the kernels can follow blindly, and the bytes the writer had
    {
        int *d_bad = nullptr, bad = 0;
        HIP_TRY(hipMalloc((void **)&d_bad, sizeof(int)));
        hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream);
        for (int c = 0; c < BSIG_MAX_CLASSES && e == hipSuccess; ++c) {
            const BsigClassCols &C = R->dev.cls[c];
            if (C.n) e = bsig::launch_check_idx(C.idx, R->idx_entries[c] - 2, (uint32_t)C.n, d_bad, ctx->stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_bad);
        if (e != hipSuccess) return fail(BSIG_ERR_DEVICE, "checking %s failed: %s", path, hipGetErrorString(e));
        if (bad) return fail(BSIG_ERR_FORMAT, "%s is damaged (bucket index)", path);
        uint64_t sum = 0;
        const int rc = layout_checksum(R.get(), &sum);
        if (rc) return rc;
        if (sum != H.checksum) return fail(BSIG_ERR_FORMAT, "%s is damaged (checksum)", path);
    }
    if (const int rc = make_packed_half(R.get(), ctx->stream)) return rc;
    *out = R.release();
    return BSIG_OK;
}

// ---------------------------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------------------------
}  // extern "C"
// The one rule for a plan's parameters: bsig_plan_create and bsig_plan_create_sum apply it, and the file-level calls
// before any decode.  Of several faults the first in this order is reported: the mode; the binsize (profile >= 1,
// coverage_ex 1 .. 65,536); the tlen filter's arity; midpoint / extend without a filter; ext < 0; ext > 2^30; threads;
// a negative width.  The overlap modes (bamOverlaps) are bamCount's family with rules of their own, asked in this order:
// minoverlap (the binsize field) >= 1; the filter's arity; no shift; no midpoint; extend needs the filter; ext as coverage's.
// frag_len (a resized plan's; resized_rule has judged it ahead of this rule) only widens ext to frag_len - 1.
int bsig::check_params(const bsig_params &prm, int64_t n, const int32_t *len, PlanRule *out, int32_t frag_len)
{
    // coverage with bins / strands IS coverage from here on (the result layout, ext, tspan, the heavy-tile ceiling);
    // only binsize, ss and cov_ex tell it apart (mode 2 ignores binsize and ss)
    PlanRule r;
    r.cov_ex = prm.mode == BSIG_MODE_COVERAGE_EX;
    r.mode = r.cov_ex ? BSIG_MODE_COVERAGE : prm.mode;
    r.overlap = prm.mode == BSIG_MODE_OVERLAP_ANY ? 1 : prm.mode == BSIG_MODE_OVERLAP_WITHIN ? 2 : 0;
    if (r.overlap) r.mode = BSIG_MODE_COUNT;
    if (r.mode != BSIG_MODE_PROFILE && r.mode != BSIG_MODE_COUNT && r.mode != BSIG_MODE_COVERAGE)
        return fail(BSIG_ERR_ARG, "unknown mode %d", r.mode);
    if ((r.mode == BSIG_MODE_PROFILE || r.cov_ex) && prm.binsize < 1)
        return fail(BSIG_ERR_ARG, "provide a binsize greater or equal to 1");       // ref: R/wrappers.R:136-137
    if (r.cov_ex && prm.binsize > kMaxCoverageBin)
        return fail(BSIG_ERR_ARG, "coverage bins are at most 65536 bases wide (bamProfile / bamCount count at that scale)");
    if (r.overlap && prm.binsize < 1) return fail(BSIG_ERR_ARG, "minoverlap must be at least 1");
    if (prm.n_tlen_filter != 0 && prm.n_tlen_filter != 2) return fail(BSIG_ERR_ARG, "tlen_filter must have 0 or 2 elements");
    if (r.overlap && prm.shift != 0) return fail(BSIG_ERR_ARG, "bamOverlaps takes no shift: a read overlaps where it lies");
    if (r.overlap && prm.pe_mid != 0) return fail(BSIG_ERR_ARG, "bamOverlaps has no midpoint rule: a fragment overlaps as a whole (extend)");
    r.mid = r.mode != BSIG_MODE_COVERAGE && prm.pe_mid;
    r.tspan = (r.mode == BSIG_MODE_COVERAGE || r.overlap) && prm.tspan;
    if ((r.mid || r.tspan) && prm.n_tlen_filter != 2)
        return fail(BSIG_ERR_ARG, "paired-end midpoint/extend needs a 2-element tlen_filter");
    // ext: ref src/bamsignals.cpp:457 (pileup) and :487 (coverage); :243 rejects negatives
    // a resized plan (resized_rule: coverage, no tspan): a read counts up to frag_len - 1 bases beyond itself, on the side
    // its strand says -- see the argument at class_window (kernels.hip)
    r.frag_len = r.mode == BSIG_MODE_COVERAGE && !r.tspan ? frag_len : 0;
    if (r.mode == BSIG_MODE_COVERAGE || r.overlap) r.ext = r.tspan ? prm.tlen_filter[1] : r.frag_len ? r.frag_len - 1 : 0;
    else r.ext = std::llabs((long long)prm.shift) + (r.mid ? (int64_t)prm.tlen_filter[1] : 0);
    if (r.ext < 0) return fail(BSIG_ERR_EXT, "negative 'ext' values don't make sense");
    if (r.ext > (1ll << 30)) return fail(BSIG_ERR_ARG, "shift / tlen filter too large");
    r.threads = prm.threads != 0 ? prm.threads : 64;
    if (r.threads != 64 && r.threads != 128 && r.threads != 256) return fail(BSIG_ERR_ARG, "threads must be 64, 128 or 256");
    for (int64_t i = 0; i < n; ++i)
        if (len[i] < 0) return fail(BSIG_ERR_ARG, "range %lld has a negative width", (long long)i);
    r.binsize = r.mode == BSIG_MODE_PROFILE || r.cov_ex ? prm.binsize : 1;
    r.ss = (r.mode != BSIG_MODE_COVERAGE || r.cov_ex) && prm.ss != 0;
    r.lay_binsize = r.mode == BSIG_MODE_COUNT ? -1 : r.binsize;
    r.minoverlap = r.overlap ? prm.binsize : 0;
    *out = r;
    return BSIG_OK;
}

// What only a resized plan asks, ahead of check_params: bamCoverage (either mode), whose reads are not already extended to
// their own template length, and a fragment length the packed class's 32-bit sums hold.
int bsig::resized_rule(const bsig_params &prm, int32_t frag_len)
{
    if (prm.mode != BSIG_MODE_COVERAGE && prm.mode != BSIG_MODE_COVERAGE_EX)
        return fail(BSIG_ERR_ARG, "reads are resized to the fragment for bamCoverage only (mode %d given)", prm.mode);
    if (prm.tspan != 0)
        return fail(BSIG_ERR_ARG, "a paired-end fragment already has its length: tspan must be 0 with a fragment length");
    if (frag_len < 1 || frag_len > BSIG_FRAG_LEN_MAX)
        return fail(BSIG_ERR_ARG, "the fragment length must be between 1 and %d (%d given)", BSIG_FRAG_LEN_MAX, frag_len);
    return BSIG_OK;
}

// bamCount and bamOverlaps: one cell per range
static bool count_family(int mode) { return mode == BSIG_MODE_COUNT || mode == BSIG_MODE_OVERLAP_ANY || mode == BSIG_MODE_OVERLAP_WITHIN; }

// What only a sum over ranges asks, ahead of check_params: no bamCount, ranges of one width.  The sum is built on per-base
// tiles; mode 2 ignores binsize and ss.
int bsig::sum_shape(const bsig_params &prm, int64_t n, const int32_t *len, SumShape *out)
{
    if (count_family(prm.mode)) return fail(BSIG_ERR_ARG, "bamCount has no sum over ranges (its sum is one number per strand)");
    for (int64_t i = 1; i < n; ++i)
        if (len[i] != len[0]) return fail(BSIG_ERR_ARG, "all signals must have the same length");     // alignSignals
    SumShape s;
    s.tiles = prm;
    s.tiles.binsize = 1;
    s.tiles.threads = 64;
    s.width = n > 0 ? len[0] : 0;
    s.binsize = prm.mode == BSIG_MODE_COVERAGE ? 1 : prm.binsize;
    s.nw = prm.threads > 0 ? prm.threads / 64 : 4;
    const int64_t S = prm.mode != BSIG_MODE_COVERAGE && prm.ss ? 2 : 1;
    // (a binsize below 1 fails check_params: no cells)
    s.cells = s.width > 0 && s.binsize > 0 ? ((int64_t)s.width + s.binsize - 1) / s.binsize * S : 0;
    *out = s;
    return BSIG_OK;
}

// What only a strand cross-correlation asks, ahead of check_params: a lag range the kernel's LDS holds, and the one
// profile the definition is stated in (per base, no shift, no midpoint; stranded by nature, so ss is not read).
int bsig::xcorr_shape(const bsig_params &prm, int32_t max_lag, XcorrShape *out)
{
    if (max_lag < 0 || max_lag > BSIG_XCORR_MAX_LAG)
        return fail(BSIG_ERR_ARG, "max_lag must be between 0 and %d", BSIG_XCORR_MAX_LAG);
    if (prm.mode != BSIG_MODE_PROFILE) return fail(BSIG_ERR_ARG, "the strand cross-correlation is defined on bamProfile (mode %d given)", prm.mode);
    if (prm.binsize != 1) return fail(BSIG_ERR_ARG, "the strand cross-correlation is per base: binsize must be 1");
    if (prm.shift != 0) return fail(BSIG_ERR_ARG, "the strand cross-correlation measures the shift: shift must be 0");
    if (prm.pe_mid) return fail(BSIG_ERR_ARG, "the strand cross-correlation has no paired-end midpoint rule");
    XcorrShape s;
    s.tiles = prm;
    s.tiles.ss = 1;
    s.tiles.threads = prm.threads != 0 ? prm.threads : 256;
    s.max_lag = max_lag;
    s.body = prm.tile_cells > 0 ? std::min(std::max(prm.tile_cells, 16), 2048) : 2048;
    s.cells = (int64_t)max_lag + 1 + BSIG_XCORR_MOMENTS;
    *out = s;
    return BSIG_OK;
}

// What only a fragment-length histogram asks, ahead of check_params: bamCount's tiles without a shift, a length filter
// (its upper end sizes the result) and as many rows as the kernel's LDS holds.  ss is not read: the range's strand does
// not influence the result.
int bsig::frag_shape(const bsig_params &prm, int32_t len_bin, FragShape *out)
{
    if (prm.mode != BSIG_MODE_COUNT) return fail(BSIG_ERR_ARG, "the fragment-length histogram is defined on bamCount (mode %d given)", prm.mode);
    if (prm.shift != 0) return fail(BSIG_ERR_ARG, "the fragment-length histogram counts unshifted positions: shift must be 0");
    if (prm.n_tlen_filter != 2) return fail(BSIG_ERR_ARG, "the fragment-length histogram needs a 2-element tlen_filter");
    if (len_bin < 1) return fail(BSIG_ERR_ARG, "len_bin must be greater or equal to 1");
    if (prm.tlen_filter[1] < 0) return fail(BSIG_ERR_ARG, "tlen_filter[1] must not be negative");
    const int64_t rows = (int64_t)prm.tlen_filter[1] / len_bin + 1;
    if (rows > BSIG_FRAG_MAX_ROWS)
        return fail(BSIG_ERR_ARG, "tlen_filter[1] / len_bin + 1 = %lld rows, at most %d fit: choose a wider len_bin", (long long)rows, BSIG_FRAG_MAX_ROWS);
    FragShape s;
    s.tiles = prm;
    s.tiles.ss = 0;
    s.tiles.pe_mid = prm.pe_mid != 0;
    s.tiles.tlen_filter[0] = std::max(prm.tlen_filter[0], 0);      // (a length is never negative: rows start at 0)
    s.tiles.threads = prm.threads != 0 ? prm.threads : 256;
    s.len_bin = len_bin;
    s.cells = rows;
    *out = s;
    return BSIG_OK;
}

// What only a V-plot asks, ahead of check_params: bamProfile's parameters without shift or strands, a length filter (its upper
// end sizes the rows), both bin widths >= 1, ranges of one width (sum_shape's rule) and a table within the caps.  Its tiles
// are a frag plan's: count tiles, which no binsize cuts.
int bsig::vplot_shape(const bsig_params &prm, int64_t n, const int32_t *len, int32_t len_bin, VplotShape *out)
{
    if (prm.mode != BSIG_MODE_PROFILE) return fail(BSIG_ERR_ARG, "the V-plot is defined on bamProfile (mode %d given)", prm.mode);
    if (prm.shift != 0) return fail(BSIG_ERR_ARG, "the V-plot counts unshifted positions: shift must be 0");
    if (prm.ss != 0) return fail(BSIG_ERR_ARG, "the V-plot has no strand split: ss must be 0");
    if (prm.n_tlen_filter != 2) return fail(BSIG_ERR_ARG, "the V-plot needs a 2-element tlen_filter");
    if (len_bin < 1) return fail(BSIG_ERR_ARG, "len_bin must be greater or equal to 1");
    if (prm.binsize < 1) return fail(BSIG_ERR_ARG, "provide a binsize greater or equal to 1");
    if (prm.tlen_filter[1] < 0) return fail(BSIG_ERR_ARG, "tlen_filter[1] must not be negative");
    SumShape widths;
    if (const int rc = sum_shape(prm, n, len, &widths)) return rc;
    const int64_t rows = (int64_t)prm.tlen_filter[1] / len_bin + 1;
    const int64_t cols = widths.width > 0 ? ((int64_t)widths.width + prm.binsize - 1) / prm.binsize : 0;
    if (rows > BSIG_FRAG_MAX_ROWS)
        return fail(BSIG_ERR_ARG, "tlen_filter[1] / len_bin + 1 = %lld rows, at most %d fit: choose a wider len_bin", (long long)rows, BSIG_FRAG_MAX_ROWS);
    if (rows * cols > BSIG_VPLOT_MAX_CELLS)
        return fail(BSIG_ERR_ARG, "%lld rows x %lld columns are more than %lld cells: choose a wider len_bin or binsize", (long long)rows,
                    (long long)cols, (long long)BSIG_VPLOT_MAX_CELLS);
    VplotShape s;
    s.tiles = prm;
    s.tiles.mode = BSIG_MODE_COUNT;
    s.tiles.binsize = -1;
    s.tiles.pe_mid = prm.pe_mid != 0;
    s.tiles.tlen_filter[0] = std::max(prm.tlen_filter[0], 0);      // (a length is never negative: rows start at 0)
    s.tiles.threads = prm.threads != 0 ? prm.threads : 256;
    s.len_bin = len_bin;
    s.binsize = prm.binsize;
    s.rows = (int32_t)rows;
    s.cols = (int32_t)cols;
    s.cells = rows * cols;
    *out = s;
    return BSIG_OK;
}

// What only a depth histogram asks, ahead of check_params: one of the two per-base signals the definition is stated in
// (5' ends per base without a shift; plain coverage, which has no strands), as many rows as the kernel's LDS holds beside
// its widest image, and a workgroup and tile the kernel is built for.
int bsig::hist_shape(const bsig_params &prm, int32_t max_value, HistShape *out)
{
    if (count_family(prm.mode)) return fail(BSIG_ERR_ARG, "the depth histogram counts per-base cells: bamCount has one cell per range");
    if (prm.mode == BSIG_MODE_COVERAGE_EX)
        return fail(BSIG_ERR_ARG, "the depth histogram of coverage is per base and unstranded: mode BSIG_MODE_COVERAGE");
    if (prm.mode == BSIG_MODE_PROFILE && prm.binsize != 1) return fail(BSIG_ERR_ARG, "the depth histogram is per base: binsize must be 1");
    if (prm.shift != 0) return fail(BSIG_ERR_ARG, "the depth histogram counts unshifted positions: shift must be 0");
    if (prm.mode == BSIG_MODE_COVERAGE && prm.ss != 0) return fail(BSIG_ERR_ARG, "the depth histogram of coverage has no strands: ss must be 0");
    if (max_value < 1 || max_value > BSIG_HIST_MAX_ROWS - 1)
        return fail(BSIG_ERR_ARG, "max_value must be between 1 and %d", BSIG_HIST_MAX_ROWS - 1);
    if (prm.threads != 0 && prm.threads != 64 && prm.threads != 128 && prm.threads != 256)
        return fail(BSIG_ERR_ARG, "threads must be 64, 128 or 256");
    if (prm.tile_cells != 0 && (prm.tile_cells < 16 || prm.tile_cells > 2048))
        return fail(BSIG_ERR_ARG, "tile_cells must be between 16 and 2048");
    HistShape s;
    s.tiles = prm;
    s.tiles.ss = prm.mode == BSIG_MODE_PROFILE && prm.ss != 0;
    s.tiles.threads = prm.threads != 0 ? prm.threads : 256;
    s.tiles.tile_cells = prm.tile_cells != 0 ? prm.tile_cells : 2048;
    s.max_value = max_value;
    s.cells = (int64_t)max_value + 1 + BSIG_HIST_MOMENTS;
    *out = s;
    return BSIG_OK;
}

// What only the per-range summaries ask, ahead of check_params: the depth histogram's parameter rule in their own words, and
// K thresholds that rise from 1.
int bsig::summary_shape(const bsig_params &prm, int32_t n_thresholds, const int32_t *thresholds, SummaryShape *out)
{
    if (count_family(prm.mode)) return fail(BSIG_ERR_ARG, "the range summary reduces per-base cells: bamCount has one cell per range");
    if (prm.mode == BSIG_MODE_COVERAGE_EX)
        return fail(BSIG_ERR_ARG, "the range summary of coverage is per base and unstranded: mode BSIG_MODE_COVERAGE");
    if (prm.mode == BSIG_MODE_PROFILE && prm.binsize != 1) return fail(BSIG_ERR_ARG, "the range summary is per base: binsize must be 1");
    if (prm.shift != 0) return fail(BSIG_ERR_ARG, "the range summary reduces unshifted positions: shift must be 0");
    if (prm.mode == BSIG_MODE_COVERAGE && prm.ss != 0) return fail(BSIG_ERR_ARG, "the range summary of coverage has no strands: ss must be 0");
    if (n_thresholds < 0 || n_thresholds > BSIG_SUMMARY_MAX_THRESHOLDS)
        return fail(BSIG_ERR_ARG, "n_thresholds must be between 0 and %d", BSIG_SUMMARY_MAX_THRESHOLDS);
    if (n_thresholds > 0 && !thresholds) return fail(BSIG_ERR_ARG, "thresholds is NULL");
    for (int k = 0; k < n_thresholds; ++k) {
        if (thresholds[k] < 1) return fail(BSIG_ERR_ARG, "thresholds must be at least 1 (%d given)", thresholds[k]);
        if (k > 0 && thresholds[k] <= thresholds[k - 1]) return fail(BSIG_ERR_ARG, "thresholds must be strictly increasing");
    }
    if (prm.threads != 0 && prm.threads != 64 && prm.threads != 128 && prm.threads != 256)
        return fail(BSIG_ERR_ARG, "threads must be 64, 128 or 256");
    if (prm.tile_cells != 0 && (prm.tile_cells < 16 || prm.tile_cells > 2048))
        return fail(BSIG_ERR_ARG, "tile_cells must be between 16 and 2048");
    SummaryShape s;
    s.tiles = prm;
    s.tiles.ss = prm.mode == BSIG_MODE_PROFILE && prm.ss != 0;
    s.tiles.threads = prm.threads != 0 ? prm.threads : 256;
    s.tiles.tile_cells = prm.tile_cells != 0 ? prm.tile_cells : 2048;
    s.S = s.tiles.ss ? 2 : 1;
    s.n_thresholds = n_thresholds;
    for (int k = 0; k < BSIG_SUMMARY_MAX_THRESHOLDS; ++k) s.thresholds[k] = k < n_thresholds ? thresholds[k] : 0;
    s.row = BSIG_SUMMARY_FIXED + n_thresholds;
    *out = s;
    return BSIG_OK;
}

// What only the scaled regions ask, ahead of check_params: the depth histogram's parameter rule in their own words, and
// 1 .. BSIG_SCALED_MAX_BINS bins.
int bsig::scaled_shape(const bsig_params &prm, int32_t n_bins, ScaledShape *out)
{
    if (count_family(prm.mode)) return fail(BSIG_ERR_ARG, "the scaled regions bin per-base cells: bamCount has one cell per range");
    if (prm.mode == BSIG_MODE_COVERAGE_EX)
        return fail(BSIG_ERR_ARG, "the scaled regions of coverage are per base and unstranded: mode BSIG_MODE_COVERAGE");
    if (prm.mode == BSIG_MODE_PROFILE && prm.binsize != 1)
        return fail(BSIG_ERR_ARG, "the scaled regions cut per-base cells into n_bins bins: binsize must be 1");
    if (prm.shift != 0) return fail(BSIG_ERR_ARG, "the scaled regions bin unshifted positions: shift must be 0");
    if (prm.mode == BSIG_MODE_COVERAGE && prm.ss != 0) return fail(BSIG_ERR_ARG, "the scaled regions of coverage have no strands: ss must be 0");
    if (n_bins < 1 || n_bins > BSIG_SCALED_MAX_BINS) return fail(BSIG_ERR_ARG, "n_bins must be between 1 and %d", BSIG_SCALED_MAX_BINS);
    if (prm.threads != 0 && prm.threads != 64 && prm.threads != 128 && prm.threads != 256)
        return fail(BSIG_ERR_ARG, "threads must be 64, 128 or 256");
    if (prm.tile_cells != 0 && (prm.tile_cells < 16 || prm.tile_cells > 2048))
        return fail(BSIG_ERR_ARG, "tile_cells must be between 16 and 2048");
    ScaledShape s;
    s.tiles = prm;
    s.tiles.ss = prm.mode == BSIG_MODE_PROFILE && prm.ss != 0;
    s.tiles.threads = prm.threads != 0 ? prm.threads : 256;
    s.tiles.tile_cells = prm.tile_cells != 0 ? prm.tile_cells : 2048;
    s.S = s.tiles.ss ? 2 : 1;
    s.n_bins = n_bins;
    *out = s;
    return BSIG_OK;
}

// What only the capped 5' ends ask, ahead of check_params: single ends on bamProfile or bamCount, and a cap of at least 1.  The
// tiles are per-base and strand-split whatever the result's bins and strands: the cap applies per base and strand.
int bsig::capped_shape(const bsig_params &prm, int32_t keep_dup, int32_t frag_len, CappedShape *out)
{
    const bool cover = prm.mode == BSIG_MODE_COVERAGE || prm.mode == BSIG_MODE_COVERAGE_EX;
    if (!cover && prm.mode != BSIG_MODE_PROFILE && prm.mode != BSIG_MODE_COUNT)
        return fail(BSIG_ERR_ARG, "keep_dup is defined on bamProfile, bamCount and bamCoverage (mode %d given)", prm.mode);
    if (cover && frag_len == 0)
        return fail(BSIG_ERR_ARG, "duplicates of different lengths have no defined survivor: bamCoverage takes keep_dup with a fragment length only");
    if (!cover && frag_len != 0)
        return fail(BSIG_ERR_ARG, "reads are resized to the fragment for bamCoverage only (mode %d given): frag_len must be 0", prm.mode);
    if (cover && (frag_len < 1 || frag_len > BSIG_FRAG_LEN_MAX))
        return fail(BSIG_ERR_ARG, "the fragment length must be between 1 and %d (%d given)", BSIG_FRAG_LEN_MAX, frag_len);
    if (keep_dup < 1) return fail(BSIG_ERR_ARG, "keep_dup must be at least 1 (%d given)", keep_dup);
    if (prm.pe_mid != 0)
        return fail(BSIG_ERR_ARG, "a paired-end duplicate is a fragment with both ends equal, which a 5' end and a strand do not identify: pe_mid must be 0 with keep_dup");
    if (prm.tspan != 0)
        return fail(BSIG_ERR_ARG, "a paired-end duplicate is a fragment with both ends equal, which a 5' end and a strand do not identify: tspan must be 0 with keep_dup");
    if (prm.n_tlen_filter != 0)
        return fail(BSIG_ERR_ARG, "keep_dup caps single-end reads: it takes no template-length rule (n_tlen_filter must be 0)");
    const bool bins = prm.mode == BSIG_MODE_PROFILE || prm.mode == BSIG_MODE_COVERAGE_EX;
    if (bins && prm.binsize < 1) return fail(BSIG_ERR_ARG, "provide a binsize greater or equal to 1");
    if (prm.mode == BSIG_MODE_COVERAGE_EX && prm.binsize > kMaxCoverageBin)
        return fail(BSIG_ERR_ARG, "coverage bins are at most 65536 bases wide (bamProfile / bamCount count at that scale)");
    if (prm.threads != 0 && prm.threads != 64 && prm.threads != 128 && prm.threads != 256)
        return fail(BSIG_ERR_ARG, "threads must be 64, 128 or 256");
    if (prm.tile_cells != 0 && (prm.tile_cells < 16 || prm.tile_cells > 2048))
        return fail(BSIG_ERR_ARG, "tile_cells must be between 16 and 2048");
    CappedShape s;
    s.tiles = prm;
    s.tiles.mode = BSIG_MODE_PROFILE;
    s.tiles.binsize = 1;
    s.tiles.ss = 1;
    if (cover) s.tiles.shift = 0;       // (coverage takes no shift)
    s.tiles.threads = prm.threads != 0 ? prm.threads : 256;
    s.tiles.tile_cells = prm.tile_cells != 0 ? prm.tile_cells : 2048;
    s.keep_dup = keep_dup;
    s.frag_len = frag_len;
    s.lay_binsize = prm.mode == BSIG_MODE_COUNT ? -1 : bins ? prm.binsize : 1;
    s.binsize = bsig::capped_binsize(s.lay_binsize);
    s.S = prm.mode != BSIG_MODE_COVERAGE && prm.ss != 0 ? 2 : 1;
    *out = s;
    return BSIG_OK;
}

static int sum_setup(bsig_plan *P, const bsig::SumShape &shape, const std::vector<BsigWorkItem> &items, const std::vector<BsigWorkItem> &hitems);
static int capped_setup(bsig_plan *P, const bsig::CappedShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide);
static int scaled_setup(bsig_plan *P, const bsig::ScaledShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide);
static int summary_setup(bsig_plan *P, const bsig::SummaryShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide);
static int hist_setup(bsig_plan *P, const bsig::HistShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide, int64_t n_cells);
static int frag_setup(bsig_plan *P, const bsig::FragShape &shape, const std::vector<int64_t> &reads_of_tile);
static int vplot_setup(bsig_plan *P, const bsig::VplotShape &shape, const std::vector<int64_t> &reads_of_tile);
static int xcorr_setup(bsig_plan *P, const bsig::XcorrShape &shape, int body, int64_t n_wide, int64_t n_cells);
// Which plan plan_create_impl is to make, and what that kind's *_shape call worked out for it:
// kSum: its tiles ordered by c0 (then by (rid, loc)), runs and slabs set up
// kXcorr: tiles of a body and an antisense halo, none of them cut into slices
// kFrag: count tiles, none of them cut into slices (they have no image)
// kVplot: a frag plan's tiles
// kHist: the mode's per-base tiles, none of them cut into slices
// kSummary, kScaled: the same tiles, each carrying its range's result row
// kCapped: per-base strand-split tiles, each carrying its range's first cell of a result laid out by the call's own bins
struct PlanRequest {
    PlanKind kind = kPlain;
    int32_t frag_len = 0;           // kPlain, kSum: a resized plan's fragment length (bsig::resized_rule passed), else 0
    union {
        const void *none = nullptr;
        const bsig::SumShape *sum;
        const bsig::XcorrShape *xcorr;
        const bsig::FragShape *frag;
        const bsig::HistShape *hist;
        const bsig::SummaryShape *summary;
        const bsig::ScaledShape *scaled;
        const bsig::VplotShape *vplot;
        const bsig::CappedShape *capped;
    };
};
// (planmath.h's pairs go to the device as uint2, byte for byte)
static_assert(sizeof(bsig::Pair32) == sizeof(uint2) && offsetof(bsig::Pair32, x) == offsetof(uint2, x) && offsetof(bsig::Pair32, y) == offsetof(uint2, y),
              "Pair32 must be laid out as uint2");
static bsig::KindFacts kind_facts(const PlanRequest &rq)
{
    bsig::KindFacts kf;
    switch (rq.kind) {
    case kPlain: break;
    case kSum: kf.sum = true; break;
    case kXcorr: kf.xcorr = true; kf.xcorr_body = rq.xcorr->body; kf.max_lag = rq.xcorr->max_lag; break;
    case kFrag: kf.frag = true; kf.len_bin = rq.frag->len_bin; break;
    // the kinds that walk their tiles whole: the caller's tile (16 .. 2,048 cells, checked by the kind's *_shape)
    case kHist: kf.own_tile_cells = rq.hist->tiles.tile_cells; break;
    case kSummary: kf.own_tile_cells = rq.summary->tiles.tile_cells; kf.row_tiles = true; break;
    case kScaled: kf.own_tile_cells = rq.scaled->tiles.tile_cells; kf.row_tiles = true; break;
    case kVplot: kf.frag = true; kf.len_bin = rq.vplot->len_bin; break;
    case kCapped: kf.own_tile_cells = rq.capped->tiles.tile_cells; kf.capped = true; break;
    }
    return kf;
}
// What plan_create_impl's stages hand on: the caller's arguments, the plan being made, and the host side of its tiles
struct PlanWork {
    bsig_ctx *ctx;
    const bsig_reads *reads;
    int64_t n;
    const int32_t *rid, *loc, *len, *strand;
    const bsig_params *prm;
    const PlanRequest &rq;
    bsig::PlanRule r{};
    bsig::KindFacts kf;
    bsig::TileSize ts{};
    std::unique_ptr<bsig_plan> plan;
    std::vector<BsigWorkItem> items;
    // probe_windows: the tiles' windows on the device; on the host (with the reads they hold, tile by tile) only when
    // somebody reads them
    DevPool tmp;
    uint2 *d_win = nullptr;
    bool any_heavy = false;
    std::vector<bsig::Pair32> win;
    std::vector<int64_t> reads_of_tile;
    int64_t heavy_reads = 0, slice_reads = 0;
    bsig::HeavySplit heavy;
    PlanWork(bsig_ctx *ctx_, const bsig_reads *reads_, int64_t n_, const int32_t *rid_, const int32_t *loc_, const int32_t *len_,
             const int32_t *strand_, const bsig_params *prm_, const PlanRequest &rq_)
        : ctx(ctx_), reads(reads_), n(n_), rid(rid_), loc(loc_), len(len_), strand(strand_), prm(prm_), rq(rq_) {}
    // a tile of these kinds is walked whole: a cell's value must be complete before it is counted or compared
    bool whole_tiles() const { return rq.kind == kHist || kf.row_tiles || kf.capped; }
    // count tiles without an image (frag, vplot): none is heavy, and their setup cuts the runs by the reads in their windows
    bool imageless() const { return kf.frag; }
};
// every HIP error of plan creation is the one refusal
static int upload_failed(hipError_t e)
{
    return fail(e == hipErrorOutOfMemory ? BSIG_ERR_NOMEM : BSIG_ERR_DEVICE, "plan upload failed: %s", hipGetErrorString(e));
}
#define PLAN_TRY(expr)                                      \
    do {                                                    \
        const hipError_t e_ = (expr);                       \
        if (e_ != hipSuccess) return upload_failed(e_);     \
    } while (0)

// What a spliced set (rows = aligned blocks, splice.hip) may be asked: the coverage of the blocks as they lie.  A block's
// start is no 5' end, a block is no fragment, and the blocks of one read would each be extended or resized: every other
// signal would be silently wrong, so its creator refuses, in its own words.
static int spliced_rule(const bsig_params &prm, const PlanRequest &rq)
{
    const bool coverage = prm.mode == BSIG_MODE_COVERAGE || prm.mode == BSIG_MODE_COVERAGE_EX;
    switch (rq.kind) {
    case kCapped: return fail(BSIG_ERR_ARG, "spliced reads: keep_dup caps reads by their 5' end, and a block's start is not one");
    case kXcorr: return fail(BSIG_ERR_ARG, "spliced reads: the strand cross-correlation is of 5' ends, and a block's start is not one");
    case kFrag: return fail(BSIG_ERR_ARG, "spliced reads: the fragment-length histogram counts reads, not their blocks");
    case kVplot: return fail(BSIG_ERR_ARG, "spliced reads: the V-plot counts reads, not their blocks");
    default: break;
    }
    if (rq.frag_len) return fail(BSIG_ERR_ARG, "spliced reads: frag_len would resize every block of a read, not the read");
    if (prm.mode == BSIG_MODE_OVERLAP_ANY || prm.mode == BSIG_MODE_OVERLAP_WITHIN)
        return fail(BSIG_ERR_ARG, "spliced reads: bamOverlaps would count a read once for each of its blocks");
    if (!coverage) return fail(BSIG_ERR_ARG, "spliced reads give coverage only: a block's start is not a read's 5' end");
    if (prm.tspan) return fail(BSIG_ERR_ARG, "spliced reads: tspan would extend every block of a read to the whole fragment");
    return BSIG_OK;
}
// stage 1: the arguments, the parameters (check_params), the chromosome ids
static int check_request(PlanWork &W, bsig_plan **out)
{
    if (!W.ctx || !W.reads || !W.prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create");
    *out = nullptr;
    if (W.n < 0 || (W.n > 0 && (!W.rid || !W.loc || !W.len || !W.strand))) return fail(BSIG_ERR_ARG, "range arrays missing");
    if (const int rc = bsig::check_params(*W.prm, W.n, W.len, &W.r, W.rq.frag_len)) return rc;
    if (W.reads->spliced)
        if (const int rc = spliced_rule(*W.prm, W.rq)) return rc;
    for (int64_t i = 0; i < W.n; ++i)
        if (W.rid[i] < 0 || W.rid[i] >= W.reads->n_ref)
            return fail(BSIG_ERR_CHROM, "chromosome id %d not present in the bam file", W.rid[i]);
    return BSIG_OK;
}
// stage 2: the plan with its tile size and its kernels' parameters (planmath.h: tile_cells_for, fill_kparams)
static void shape_plan(PlanWork &W)
{
    const bsig_reads *reads = W.reads;
    W.plan.reset(new bsig_plan);
    bsig_plan *P = W.plan.get();
    P->ctx = W.ctx; P->reads = reads; P->mode = W.r.mode; P->n_ranges = W.n;
    P->made_for_gen = reads->layout_gen;
    P->threads = W.r.threads;
    W.kf = kind_facts(W.rq);
    W.ts = bsig::tile_cells_for(W.r, W.prm->tile_cells, W.n, W.len, W.kf);
    P->tile_cells = W.ts.cells;
    bsig::LayoutFacts L{};
    const uint16_t *packed = reads->dev.cls[BSIG_CLASS_PACKED].p5h;
    for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
        const BsigClassCols &C = reads->dev.cls[c];
        L.cls[c] = bsig::ClassFacts{C.n, C.maxspan, C.kshift, C.p5h != nullptr, C.p5h && packed ? (uint32_t)(C.p5h - packed) : 0u};
    }
    L.codes = reads->fmtab.data();
    L.n_codes = reads->dev.n_codes;
    const char *quad = getenv("BAMSIGNALS_OVERLAP_QUAD");
    bsig::fill_kparams(P->kp, *W.prm, W.r, P->tile_cells, L, W.kf, quad && !strcmp(quad, "0"));
}
// stage 3: the result's layout, the ranges in genomic order (ref: std::sort by (rid, loc), src/bamsignals.cpp:222-226,246)
// and their tiles (planmath.h: cut_tiles)
static int cut_plan(PlanWork &W)
{
    bsig_plan *P = W.plan.get();
    P->off.resize(W.n + 1);
    // (a capped plan's tiles are per base and strand-split; its result has the call's own bins and strands)
    // ... and the capped coverage's tiles store the capped ends of the widened ranges into the plan's scratch, laid out here
    if (W.rq.kind == kCapped && W.rq.capped->frag_len) bsig_layout(W.n, W.len, 1, 1, P->off.data());
    else if (W.rq.kind == kCapped) bsig_layout(W.n, W.len, W.rq.capped->lay_binsize, W.rq.capped->S == 2, P->off.data());
    else bsig_layout(W.n, W.len, W.r.lay_binsize, P->kp.ss, P->off.data());
    std::vector<int64_t> order;
    bsig::sort_ranges(W.n, W.rid, W.loc, order);
    bsig::Tiles T = bsig::cut_tiles(order, W.rid, W.loc, W.len, W.strand, P->off.data(), W.reads->ref_unit0.data(),
                                    W.reads->ref_units.data(), W.r, W.prm->tile_cells, W.ts, W.kf);
    W.items = std::move(T.items);
    P->needs_zero = T.needs_zero;
    P->kernel_mode = T.kernel_mode;
    P->n_items = (int64_t)W.items.size();
    if (P->n_items >= (1ll << 31)) return fail(BSIG_ERR_ARG, "too many tiles for one launch");
    return BSIG_OK;
}
// stage 4: the tiles and the packed class's filter table for these parameters (kernels.hip: k_make_ptab) on the device
static int upload_tiles(PlanWork &W)
{
    bsig_plan *P = W.plan.get();
    hipStream_t st = W.ctx->stream;
    PLAN_TRY(hipSetDevice(W.ctx->device));
    PLAN_TRY(P->pool.alloc(&P->items, std::max<size_t>(W.items.size(), 1)));
    PLAN_TRY(P->pool.alloc(&P->ptab, (size_t)BSIG_PACK_CODES));
    PLAN_TRY(bsig::launch_make_ptab(W.reads->dev, P->kp, P->ptab, st));
    P->kp.ptab = P->ptab;
    if (!W.items.empty()) PLAN_TRY(hipMemcpyAsync(P->items, W.items.data(), W.items.size() * sizeof(BsigWorkItem), hipMemcpyHostToDevice, st));
    PLAN_TRY(hipStreamSynchronize(st));
    return BSIG_OK;
}
// stage 5: One wave streams a tile's reads; a tile on a read hotspot (chrM, rDNA, an amplicon) can hold millions and would
// keep the whole launch waiting.  The window sizes are probed once per plan; the windows themselves are only fetched when
// there is something to slice (a frag plan cuts its runs by them, the kinds that walk their tiles whole prove their sums
// by them).
static int probe_windows(PlanWork &W)
{
    bsig_plan *P = W.plan.get();
    hipStream_t st = W.ctx->stream;
    W.heavy_reads = 32768; W.slice_reads = 8192;
    // (k_profile's 16-bit tile image relies on the 32,768 ceiling: the environment may only lower it)
    if (const char *v = getenv("BAMSIGNALS_HEAVY_READS")) {
        W.heavy_reads = std::min<long long>(32768, std::max<long long>(4, atoll(v)));
        W.slice_reads = std::max<int64_t>(4, W.heavy_reads / 4);
    }
    // (k_coverage's cells are SIGNED 16-bit: +32,768 starts on one cell would not fit; k_coverage_bins' int32 cells
    // need the same ceiling: 32,767 reads adding at most 65,536 each stay below 2^31)
    if (P->kernel_mode == BSIG_MODE_COVERAGE) W.heavy_reads = std::min<int64_t>(W.heavy_reads, 32767);
    if (W.items.empty()) return BSIG_OK;
    unsigned long long *d_heavy = nullptr, n_heavy_dev = 0;
    PLAN_TRY(W.tmp.alloc(&W.d_win, W.items.size() * BSIG_MAX_CLASSES));
    PLAN_TRY(W.tmp.alloc(&d_heavy, 1));
    PLAN_TRY(hipMemsetAsync(d_heavy, 0, sizeof(unsigned long long), st));
    PLAN_TRY(bsig::launch_resolve(W.reads->dev, P->kp, P->kernel_mode, P->items, P->n_items, W.d_win, st));
    PLAN_TRY(bsig::launch_count_heavy(W.d_win, P->n_items, W.heavy_reads, d_heavy, st));
    PLAN_TRY(hipMemcpyAsync(&n_heavy_dev, d_heavy, sizeof n_heavy_dev, hipMemcpyDeviceToHost, st));
    PLAN_TRY(hipStreamSynchronize(st));
    // a tile of a fragment-length histogram or a V-plot has no image that its reads could overflow: none is heavy, none is sliced
    W.any_heavy = n_heavy_dev != 0 && !W.imageless();
    if (!n_heavy_dev && !W.imageless() && !W.whole_tiles()) return BSIG_OK;
    W.win.resize(W.items.size() * BSIG_MAX_CLASSES);
    PLAN_TRY(hipMemcpyAsync(W.win.data(), W.d_win, W.win.size() * sizeof(uint2), hipMemcpyDeviceToHost, st));
    PLAN_TRY(hipStreamSynchronize(st));
    W.reads_of_tile = bsig::reads_of_tiles(W.win);
    return BSIG_OK;
}
// stage 6: the proofs that no 64-bit sum of a plan whose tiles are walked whole wraps (planmath.h: depth_bound) -- the depth
// histogram's over all tiles, the summaries' range by range (a range's tiles are consecutive, and out_off is its row)
static int check_depth_bounds(const PlanWork &W)
{
    if (W.reads_of_tile.empty() || !W.whole_tiles()) return BSIG_OK;
    const std::vector<BsigWorkItem> &items = W.items;
    const bool coverage = W.r.mode == BSIG_MODE_COVERAGE;
    if (!W.kf.row_tiles) {
        const long double bound = bsig::depth_bound(items, W.reads_of_tile, 0, items.size(), coverage);
        if (bound >= bsig::kTwo63)
            return fail(BSIG_ERR_ARG, "the summed depth of these ranges could exceed 2^63 - 1 (the reads of their tiles add up "
                                      "to %.3Lg): take fewer ranges per call", bound);
        return BSIG_OK;
    }
    for (size_t t = 0, u = 0; t < items.size(); t = u) {
        while (u < items.size() && items[u].out_off == items[t].out_off) ++u;
        const long double bound = bsig::depth_bound(items, W.reads_of_tile, t, u, coverage);
        if (bound >= bsig::kTwo63)
            return fail(BSIG_ERR_ARG, "the summed depth of range %lld could exceed 2^63 - 1 (the reads of its tiles add up "
                                      "to %.3Lg): cut the range", (long long)(items[t].out_off / (W.r.ss ? 2 : 1)), bound);
    }
    return BSIG_OK;
}
// stage 7: the heavy tiles cut into slices or marked to be walked whole (planmath.h: split_heavy), their items and windows
// uploaded, the main items once more with their heavy flags
static int upload_heavy(PlanWork &W)
{
    bsig_plan *P = W.plan.get();
    if (!W.any_heavy) return BSIG_OK;
    const bsig::HeavyPolicy policy = W.whole_tiles() || W.rq.kind == kXcorr ? bsig::kWalkWhole : bsig::kSlice;
    W.heavy = bsig::split_heavy(W.items, W.win, W.reads_of_tile, W.heavy_reads, W.slice_reads, policy, P->kernel_mode == BSIG_MODE_COUNT);
    const std::vector<BsigWorkItem> &hitems = W.heavy.hitems;
    const std::vector<bsig::Pair32> &hwin = W.heavy.hwin;
    P->n_heavy_tiles = W.heavy.n_heavy_tiles;
    if (hitems.empty()) return BSIG_OK;
    hipStream_t st = W.ctx->stream;
    P->n_heavy_slices = (int64_t)hitems.size();
    uint2 *hw = nullptr;
    PLAN_TRY(P->pool.alloc(&P->heavy_items, hitems.size()));
    if (!hwin.empty()) PLAN_TRY(P->pool.alloc(&hw, hwin.size()));
    P->heavy_windows = hw;
    PLAN_TRY(hipMemcpyAsync(P->heavy_items, hitems.data(), hitems.size() * sizeof(BsigWorkItem), hipMemcpyHostToDevice, st));
    if (hw) PLAN_TRY(hipMemcpyAsync(hw, hwin.data(), hwin.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    // the heavy flags of the main items
    PLAN_TRY(hipMemcpyAsync(P->items, W.items.data(), W.items.size() * sizeof(BsigWorkItem), hipMemcpyHostToDevice, st));
    // binned coverage: the slices' atomic adds are the only ones that can take a bin past INT32_MAX
    if (W.r.cov_ex) {
        PLAN_TRY(P->pool.alloc(&P->overflow, 1));
        PLAN_TRY(hipMemsetAsync(P->overflow, 0, sizeof(int32_t), st));
    }
    P->kp.overflow = P->overflow;
    PLAN_TRY(hipStreamSynchronize(st));
    return BSIG_OK;
}
// ... and the cross-correlation's proof that no 64-bit sum wraps (planmath.h: xcorr_bound), which counts the heavy tiles
static int check_xcorr_bound(const PlanWork &W)
{
    if (W.rq.kind != kXcorr || W.items.empty()) return BSIG_OK;
    const long double bound = bsig::xcorr_bound(W.plan->n_items, W.plan->n_heavy_tiles, W.heavy.heavy_sq);
    if (bound >= bsig::kTwo63)
        return fail(BSIG_ERR_ARG, "the cross-correlation of these ranges could exceed 2^63 - 1 (the squared read counts "
                                  "of their tiles add up to %.3Lg): correlate fewer ranges per call", bound);
    return BSIG_OK;
}
// stage 8: what the plan's kind keeps beside its tiles
static int setup_kind(PlanWork &W)
{
    bsig_plan *P = W.plan.get();
    const PlanRequest &rq = W.rq;
    P->kind = rq.kind;
    if (rq.kind != kPlain) P->red.reset(new Reduced);
    int64_t widths = 0;             // (moments[0] of an xcorr plan; with strands twice that many cells for a hist plan's)
    for (int64_t i = 0; i < W.n; ++i) widths += W.len[i];
    const int64_t n_wide = (int64_t)W.heavy.hitems.size();
    switch (rq.kind) {
    case kPlain: break;
    case kSum: return sum_setup(P, *rq.sum, W.items, W.heavy.hitems);
    case kXcorr: return xcorr_setup(P, *rq.xcorr, W.ts.xbody, n_wide, widths);
    case kFrag: return frag_setup(P, *rq.frag, W.reads_of_tile);
    case kHist: return hist_setup(P, *rq.hist, W.items, n_wide, widths * (W.r.ss ? 2 : 1));
    case kSummary: return summary_setup(P, *rq.summary, W.items, n_wide);
    case kScaled: return scaled_setup(P, *rq.scaled, W.items, n_wide);
    case kVplot: return vplot_setup(P, *rq.vplot, W.reads_of_tile);
    case kCapped: return capped_setup(P, *rq.capped, W.items, n_wide);
    }
    return BSIG_OK;
}
// Every plan is made here, in these stages; their order is the order in which refusals win.
static int plan_create_impl(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid,
                            const int32_t *loc, const int32_t *len, const int32_t *strand,
                            const bsig_params *prm, const PlanRequest &rq, bsig_plan **out)
{
    PlanWork W(ctx, reads, n, rid, loc, len, strand, prm, rq);
    if (const int rc = check_request(W, out)) return rc;
    shape_plan(W);
    if (const int rc = cut_plan(W)) return rc;
    if (const int rc = upload_tiles(W)) return rc;
    if (const int rc = probe_windows(W)) return rc;
    if (const int rc = check_depth_bounds(W)) return rc;
    if (const int rc = upload_heavy(W)) return rc;
    if (const int rc = check_xcorr_bound(W)) return rc;
    W.tmp.release();                // (the probe's windows: not held while the kind allocates its own)
    if (const int rc = setup_kind(W)) return rc;
    *out = W.plan.release();
    return BSIG_OK;
}
// ---- what the eight *_setup functions share ------------------------------------------------------------------------
// the device's compute units and the LDS a workgroup may hold
static int device_limits(const bsig_plan *P, int *n_cu, int *lds_max)
{
    HIP_TRY(hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, P->ctx->device));
    HIP_TRY(hipDeviceGetAttribute(lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, P->ctx->device));
    return BSIG_OK;
}
// Tiles per run: as many runs as workgroups are resident at a time (`per_cu` a CU, by occupancy), so that one round of
// workgroups walks the whole plan, and at least `least` tiles a run -- unless env `name` > 0 says otherwise (tests: read
// when the plan is made)
static int64_t tiles_per_run(const bsig_plan *P, int n_cu, int per_cu, int64_t least, const char *name)
{
    if (const char *v = getenv(name)) {
        const long long forced = atoll(v);
        if (forced > 0) return forced;
    }
    const int64_t resident = (int64_t)std::max(n_cu, 1) * per_cu;
    return std::max<int64_t>(least, (P->n_items + resident - 1) / resident);
}
// (the cutters themselves -- cut_runs, append_wide_runs, cut_sum_runs -- are planmath.h's)
static int upload_runs(bsig_plan *P, const std::vector<bsig::Pair32> &runs)
{
    if (runs.empty()) return BSIG_OK;
    hipStream_t st = P->ctx->stream;
    HIP_TRY(P->pool.alloc(&P->red->runs, runs.size()));
    HIP_TRY(hipMemcpyAsync(P->red->runs, runs.data(), runs.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BSIG_OK;
}
// a lowered ceiling for what a run's 32-bit counters see (tests: env `name`, read when the plan is made)
constexpr int64_t kCounterMax = 4294967295ll;
static int64_t counter_ceiling(const char *name)
{
    const char *v = getenv(name);
    return v ? std::min<long long>(kCounterMax, std::max<long long>(1, atoll(v))) : kCounterMax;
}
// What the setup of every kind but sum ends with.  `lds` bytes are what its launches ask of a workgroup: more than the device
// has and there is no plan (refuse(lds_max) words the kind's refusal).  Then the tiles are cut into runs -- tiles_per_run
// by the occupancy of `form`, the main launch's, and env `run_tiles`; cut_runs' `ceiling` and `weight` --, the n_wide wide
// tiles follow as runs of their own, and the runs go to the device.
template <typename Refuse, typename Weight>
static int setup_runs(bsig_plan *P, size_t lds, Refuse &&refuse, const bsig::TileForm &form, const char *run_tiles, int64_t ceiling,
                      Weight &&weight, int64_t n_wide)
{
    int n_cu = 0, lds_max = 0;
    if (const int rc = device_limits(P, &n_cu, &lds_max)) return rc;
    if (lds > (size_t)lds_max) return refuse(lds_max);
    const int64_t per = tiles_per_run(P, n_cu, bsig::tile_blocks_per_cu(form), 1, run_tiles);
    std::vector<bsig::Pair32> runs;
    bsig::cut_runs(P->n_items, per, ceiling, weight, runs);
    P->red->n_runs_main = (int64_t)runs.size();
    bsig::append_wide_runs(n_wide, runs);
    P->red->n_runs_extra = n_wide;
    return upload_runs(P, runs);
}

// The runs of a sum plan: tiles of one c0 cut into runs of at most `per` (a workgroup each, one slab each), the runs of
// the heavy slices behind those of the main tiles; chunks of at most kSumChunkSlots slabs of one c0 for k_sum_reduce.
// `per` fills the chip once (workgroups resident at a time, by occupancy) and never exceeds 65,536 tiles, which keeps
// every slab exact in 32 bits (k_sum_tiles).
static int sum_setup(bsig_plan *P, const bsig::SumShape &shape, const std::vector<BsigWorkItem> &items, const std::vector<BsigWorkItem> &hitems)
{
    constexpr int64_t kMaxRunTiles = 65536;
    Reduced &R = *P->red;
    auto &Q = R.sum;
    R.cells = shape.cells;
    Q.width = shape.width; Q.binsize = shape.binsize; Q.nw = shape.nw;
    Q.S = P->kp.ss ? 2 : 1;
    Q.kind = P->kernel_mode == BSIG_MODE_PROFILE ? kSumProfile : P->kp.ss ? kSumCoverSS : kSumCover;
    Q.slab_vals = (P->tile_cells * Q.S + 3) & ~3;
    int n_cu = 0, lds_max = 0;
    if (const int rc = device_limits(P, &n_cu, &lds_max)) return rc;
    // The accumulator and one image per wave must fit a workgroup's LDS (a tile size of the caller's can ask for more:
    // strand-split coverage, 4,096 cells, four waves = 160.5 KiB): fewer waves per workgroup, and if one is too many,
    // no plan.  The library's own tile sizes (at most 2,048 cells, 1,024 with strands) need 40.5 KiB at most.
    int &nw = Q.nw;
    // (the occupancy of the form that runs on looked-up windows, not resized: all forms of a kind and nw ask for the same LDS)
    const auto form = [&] { return bsig::sum_form(Q.kind, Q.S == 2, nw, P->kp.packed_half != 0, true, false, P->tile_cells); };
    while (nw > 1 && form().lds > (size_t)lds_max) nw /= 2;
    if (form().lds > (size_t)lds_max)
        return fail(BSIG_ERR_ARG, "tile_cells %d needs %zu bytes of LDS per workgroup, the device has %d", P->tile_cells, form().lds, lds_max);
    // (BAMSIGNALS_SUM_RUN_TILES: shorter or longer runs, never past the cap that keeps a slab exact)
    const int64_t per = std::min<int64_t>(kMaxRunTiles, tiles_per_run(P, n_cu, bsig::tile_blocks_per_cu(form()), nw, "BAMSIGNALS_SUM_RUN_TILES"));
    std::vector<bsig::Pair32> runs;
    std::vector<BsigSumChunk> chunks;
    Q.max_nvals = std::max(Q.max_nvals, bsig::cut_sum_runs(items, per, Q.S, runs, chunks));
    R.n_runs_main = (int64_t)runs.size();
    Q.max_nvals = std::max(Q.max_nvals, bsig::cut_sum_runs(hitems, per, Q.S, runs, chunks));
    R.n_runs_extra = (int64_t)runs.size() - R.n_runs_main;
    Q.n_chunks = (int64_t)chunks.size();
    hipStream_t st = P->ctx->stream;
    if (!runs.empty()) {
        HIP_TRY(P->pool.alloc(&Q.chunks, chunks.size()));
        HIP_TRY(P->pool.alloc(&Q.slab, runs.size() * (size_t)Q.slab_vals));
        HIP_TRY(hipMemcpyAsync(Q.chunks, chunks.data(), chunks.size() * sizeof(BsigSumChunk), hipMemcpyHostToDevice, st));
    }
    if (shape.binsize != 1 && shape.width > 0) HIP_TRY(P->pool.alloc(&Q.base, (size_t)shape.width * Q.S));
    return upload_runs(P, runs);            // (waits for the chunks as well: one stream)
}

// The runs of an xcorr plan: the tiles, in genomic order, cut into as many runs as workgroups are resident at a time (by
// occupancy), so that one round of workgroups walks the whole plan and each keeps its per-lag sums in LDS across its run
// -- a whole-genome call then ends in one 64-bit atomic per lag and workgroup instead of one per lag and tile.
static int xcorr_setup(bsig_plan *P, const bsig::XcorrShape &shape, int body, int64_t n_wide, int64_t n_cells)
{
    Reduced &R = *P->red;
    R.cells = shape.cells;
    R.xcorr.body = body;
    R.xcorr.max_lag = shape.max_lag;
    R.xcorr.n_cells = n_cells;
    const auto form = [&](bool wide) { return bsig::xcorr_form(P->threads, P->kp.packed_half != 0, wide, P->tile_cells, body, shape.max_lag); };
    const size_t lds = form(n_wide > 0).lds;
    const auto refuse = [&](int lds_max) {
        return fail(BSIG_ERR_ARG, "a tile of %d + %d cells needs %zu bytes of LDS per workgroup, the device has %d", body,
                    shape.max_lag, lds, lds_max);
    };
    // (no counter of a run can wrap: check_xcorr_bound's proof)
    return setup_runs(P, lds, refuse, form(false), "BAMSIGNALS_XCORR_RUN_TILES", 0, [](int64_t) { return (int64_t)0; }, n_wide);
}

// The runs of a frag plan: cut as an xcorr plan's are -- a workgroup keeps its histogram in LDS across its run and ends
// with one 64-bit atomic per non-zero row.  The histogram's counters have 32 bits and every read in a tile's windows adds
// at most 1 to one of them, so a run also ends where the reads in its tiles' windows would pass the ceiling of 2^32 - 1
// (tests: BAMSIGNALS_FRAG_FLUSH_READS lowers it): no counter wraps.  (A single tile cannot hold that many: its windows are
// index ranges of 32 bits in five classes, and the plan refuses the one that would.)
static int frag_setup(bsig_plan *P, const bsig::FragShape &shape, const std::vector<int64_t> &reads_of_tile)
{
    Reduced &R = *P->red;
    auto &Q = R.frag;
    R.cells = shape.cells;
    Q.len_bin = shape.len_bin;
    // The form: one LDS atomic per accepted read ("plain", the default), or the rows equal to the wave's first accepted
    // lane's merged before it ("merge").  The merging form becomes the default only where scripts/fragsizes_times.py
    // shows it faster than the plain one by more than the runs' spread: BAMSIGNALS_FRAG_FORM chooses, read
    // when the plan is made.
    if (const char *v = getenv("BAMSIGNALS_FRAG_FORM")) Q.merge = strcmp(v, "merge") == 0;
    for (const int64_t nr : reads_of_tile)
        if (nr > kCounterMax)
            return fail(BSIG_ERR_ARG, "a tile of these ranges sees %lld reads, more than a 32-bit counter holds", (long long)nr);
    const bsig::TileForm form = bsig::frag_form(P->threads, Q.merge, (int)shape.cells);
    const auto refuse = [&](int lds_max) {
        return fail(BSIG_ERR_ARG, "%lld rows need %zu bytes of LDS per workgroup, the device has %d", (long long)shape.cells, form.lds, lds_max);
    };
    return setup_runs(P, form.lds, refuse, form, "BAMSIGNALS_FRAG_RUN_TILES", counter_ceiling("BAMSIGNALS_FRAG_FLUSH_READS"),
                      [&](int64_t t) { return reads_of_tile[(size_t)t]; }, 0);
}

// The runs of a vplot plan: a frag plan's tiles, cut as a frag plan's are.  The form: the whole table of rows x cols 32-bit
// counters in a workgroup's LDS where it fits the budget ("lds": every read in a tile's windows adds at most 1, so a run ends
// before the reads in its windows pass the ceiling of 2^32 - 1 -- tests: BAMSIGNALS_VPLOT_FLUSH_READS lowers it), else one
// 64-bit global atomic per accepted read ("global": no counter can wrap, run length only balances work).  The budget is
// all the LDS the device gives a workgroup, 160 KiB on gfx950 (40,960 counters; one workgroup a CU then): measured, a table
// of 201 x 201 cells takes 0.38 ms in LDS and 1.54 ms with global atomics, one of 201 x 101 0.21 against 2.40 ms, where the
// 64 KiB the other reductions stop at would have sent both to the global form (scripts/vplot_times.py).
// BAMSIGNALS_VPLOT_LDS_KIB lowers the budget for that comparison, BAMSIGNALS_VPLOT_FORM=global forces the global form; both
// are read when the plan is made.
static int vplot_setup(bsig_plan *P, const bsig::VplotShape &shape, const std::vector<int64_t> &reads_of_tile)
{
    Reduced &R = *P->red;
    auto &Q = R.vplot;
    R.cells = shape.cells;
    Q.rows = shape.rows; Q.cols = shape.cols;
    Q.len_bin = shape.len_bin; Q.binsize = shape.binsize;
    bsig::magic_u31(shape.binsize, &Q.bin_magic, &Q.bin_shift);
    int n_cu = 0, lds_max = 0;
    if (const int rc = device_limits(P, &n_cu, &lds_max)) return rc;
    long long budget = lds_max;
    if (const char *v = getenv("BAMSIGNALS_VPLOT_LDS_KIB")) budget = std::max<long long>(1, atoll(v)) * 1024;
    Q.lds_budget = (size_t)std::min<long long>(budget, lds_max);
    const char *forced = getenv("BAMSIGNALS_VPLOT_FORM");
    const bool global = (forced && !strcmp(forced, "global")) || (size_t)shape.cells * 4 > Q.lds_budget;
    Q.form = global ? 1 : 0;
    // one atomic per accepted read ("plain", the default), or the cells equal to the wave's first accepted lane's merged
    // before it: BAMSIGNALS_VPLOT_MERGE=1, read when the plan is made.  scripts/vplot_times.py compares the two in both
    // forms; the merging one becomes the default only where it is faster by more than the runs' spread, and it is not: in
    // LDS it measured 17 - 19 % slower, with global atomics within 2 % of the plain form on either side.
    if (const char *v = getenv("BAMSIGNALS_VPLOT_MERGE")) Q.merge = strcmp(v, "1") == 0;
    for (const int64_t nr : reads_of_tile)
        if (!global && nr > kCounterMax)
            return fail(BSIG_ERR_ARG, "a tile of these ranges sees %lld reads, more than a 32-bit counter holds", (long long)nr);
    const bsig::TileForm form = bsig::vplot_form(P->threads, global, Q.merge, (int)shape.cells, Q.lds_budget);
    const auto refuse = [&](int lds_have) {
        return fail(BSIG_ERR_ARG, "%lld cells need %zu bytes of LDS per workgroup, the device has %d", (long long)shape.cells, form.lds, lds_have);
    };
    if (global) return setup_runs(P, form.lds, refuse, form, "BAMSIGNALS_VPLOT_RUN_TILES", 0, [](int64_t) { return (int64_t)0; }, 0);
    return setup_runs(P, form.lds, refuse, form, "BAMSIGNALS_VPLOT_RUN_TILES", counter_ceiling("BAMSIGNALS_VPLOT_FLUSH_READS"),
                      [&](int64_t t) { return reads_of_tile[(size_t)t]; }, 0);
}

// The runs of a hist plan: cut as a frag plan's are.  Every cell of a tile adds 1 to one of the histogram's 32-bit
// counters, so a run also ends where the cells of its tiles would pass the ceiling of 2^32 - 1 (tests:
// BAMSIGNALS_HIST_FLUSH_CELLS lowers it; a tile holds at most 2 x 2,048 cells): no counter wraps.
static int hist_setup(bsig_plan *P, const bsig::HistShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide, int64_t n_cells)
{
    Reduced &R = *P->red;
    auto &Q = R.hist;
    R.cells = shape.cells;
    Q.max_value = shape.max_value;
    Q.coverage = P->mode == BSIG_MODE_COVERAGE;
    Q.n_cells = n_cells;
    // The form: one LDS atomic per cell ("plain", the default), or the zero cells of a wave counted by ballot and the rows
    // equal to the wave's first non-zero lane's merged before the atomic ("merge").  The merging form becomes the default
    // only where scripts/depthhist_times.py shows it faster than the plain one by more than the runs' spread:
    // BAMSIGNALS_HIST_FORM chooses, read when the plan is made.
    if (const char *v = getenv("BAMSIGNALS_HIST_FORM")) Q.merge = strcmp(v, "merge") == 0;
    const int n_rows = shape.max_value + 1;
    const auto form = [&](bool wide) { return bsig::hist_form(P->threads, Q.coverage, P->kp.packed_half != 0, wide, Q.merge, P->tile_cells, n_rows); };
    const size_t lds = form(n_wide > 0).lds;
    const auto refuse = [&](int lds_max) {
        return fail(BSIG_ERR_ARG, "%d rows and a tile of %d cells need %zu bytes of LDS per workgroup, the device has %d", n_rows,
                    P->tile_cells, lds, lds_max);
    };
    const int64_t S = P->kp.ss ? 2 : 1;
    return setup_runs(P, lds, refuse, form(false), "BAMSIGNALS_HIST_RUN_TILES", counter_ceiling("BAMSIGNALS_HIST_FLUSH_CELLS"),
                      [&](int64_t t) { return (int64_t)items[(size_t)t].nc * S; }, n_wide);
}

// The runs of a summary plan: cut as a hist plan's are.  A lane's 32-bit threshold counters grow by at most the cells its
// workgroup walks between two flushes, so a run also ends where the cells of its tiles would pass the ceiling of 2^32 - 1
// (a tile holds at most 2,048 cells): no counter wraps.  A run may hold many ranges (a flush at every change of range) or a
// part of one (the rows are combined with 64-bit atomics).
static int summary_setup(bsig_plan *P, const bsig::SummaryShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide)
{
    Reduced &R = *P->red;
    auto &Q = R.summary;
    Q.coverage = P->mode == BSIG_MODE_COVERAGE;
    Q.S = shape.S;
    R.cells = P->n_ranges * shape.S * shape.row;
    Q.thr.k = shape.n_thresholds;
    for (int k = 0; k < BSIG_SUMMARY_MAX_THRESHOLDS; ++k) Q.thr.t[k] = k < shape.n_thresholds ? (uint32_t)shape.thresholds[k] : 0xFFFFFFFFu;
    const auto form = [&](bool wide) { return bsig::summary_form(P->threads, Q.coverage, P->kp.packed_half != 0, wide, P->tile_cells); };
    const size_t lds = form(n_wide > 0).lds;
    const auto refuse = [&](int lds_max) {
        return fail(BSIG_ERR_ARG, "a tile of %d cells needs %zu bytes of LDS per workgroup, the device has %d", P->tile_cells, lds, lds_max);
    };
    return setup_runs(P, lds, refuse, form(false), "BAMSIGNALS_SUMMARY_RUN_TILES", kCounterMax,
                      [&](int64_t t) { return (int64_t)items[(size_t)t].nc; }, n_wide);
}

// The runs of a scaled plan: cut as a summary plan's are.  Its accumulators are 64 bits wide everywhere, so nothing but the
// shared cutter's ceiling bounds a run.  A workgroup holds S * N qwords of LDS beside its image.  The segmented consumer is
// chosen per plan: for coverage whose cells lie mostly in ranges with bins of 256 cells or more -- in the coverage walk a
// lane owns four consecutive cells, so one wave step spans 256 cells, and from that bin size on most steps lie inside one
// bin and take the segmented form's short path -- the one shape class where it measured faster than the plain form
// ("Scaled regions"); narrower bins put every wave on the twelve-shuffle scan, and 5' ends are mostly zeros,
// which the plain form skips.  bsig_plan_scaled_segmented() says which form a plan took.  Env
// BAMSIGNALS_SCALED_SEGMENTED (0 / 1, read when the plan is made) forces either form.
static int scaled_setup(bsig_plan *P, const bsig::ScaledShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide)
{
    Reduced &R = *P->red;
    auto &Q = R.scaled;
    Q.coverage = P->mode == BSIG_MODE_COVERAGE;
    Q.S = shape.S;
    Q.n_bins = shape.n_bins;
    R.cells = P->n_ranges * shape.S * shape.n_bins;
    int64_t cells = 0, wide_cells = 0;
    for (const BsigWorkItem &w : items) {
        cells += w.nc;
        if ((int64_t)w.len >= 256ll * shape.n_bins) wide_cells += w.nc;
    }
    Q.segmented = Q.coverage && 2 * wide_cells > cells;
    if (const char *v = getenv("BAMSIGNALS_SCALED_SEGMENTED")) Q.segmented = atoi(v) != 0;
    const auto form = [&](bool wide) {
        return bsig::scaled_form(P->threads, Q.coverage, P->kp.packed_half != 0, wide, Q.segmented, P->tile_cells, Q.S, Q.n_bins);
    };
    const size_t lds = form(n_wide > 0).lds;
    const auto refuse = [&](int lds_max) {
        return fail(BSIG_ERR_ARG, "a tile of %d cells and %d bins need %zu bytes of LDS per workgroup, the device has %d", P->tile_cells,
                    Q.n_bins, lds, lds_max);
    };
    return setup_runs(P, lds, refuse, form(false), "BAMSIGNALS_SCALED_RUN_TILES", kCounterMax,
                      [&](int64_t t) { return (int64_t)items[(size_t)t].nc; }, n_wide);
}

// The runs of a capped plan: cut as a summary plan's are, with the tiles-per-run rule of the other kinds that walk their tiles
// whole (env BAMSIGNALS_CAPPED_RUN_TILES); the wide tiles follow as runs of their own.  With bins a workgroup holds S * n_acc
// int32 accumulators of LDS beside its image, flushed after every tile: nothing but the shared cutter's ceiling bounds a run.
static int capped_setup(bsig_plan *P, const bsig::CappedShape &shape, const std::vector<BsigWorkItem> &items, int64_t n_wide)
{
    Reduced &R = *P->red;
    auto &Q = R.capped;
    Q.keep_dup = shape.keep_dup;
    Q.S = shape.S;
    Q.binned = shape.binsize > 1;
    Q.frag_len = shape.frag_len;
    bsig::magic_u31(shape.binsize, &Q.bin_magic, &Q.bin_shift);
    const bool cover = shape.frag_len > 0;
    // (the capped coverage's tiles store per-base cells with strands, whatever the result's bins: no accumulators)
    Q.n_acc = cover ? 0 : bsig::capped_tile_bins(P->tile_cells, shape.binsize);
    R.cells = P->off.back();
    if (cover) {
        const int64_t n = P->n_ranges;
        Q.res_off.resize((size_t)n + 1);
        bsig_layout(n, shape.len0, shape.lay_binsize, shape.S == 2, Q.res_off.data());
        R.cells = Q.res_off.back();
        std::vector<BsigCappedRange> rg((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t w = std::max(shape.len0[i], 0);
            rg[(size_t)i] = BsigCappedRange{P->off[(size_t)i], Q.res_off[(size_t)i], w, shape.lead[i],
                                            (int32_t)((P->off[(size_t)i + 1] - P->off[(size_t)i]) / 2), shape.strand0[i] < 0 ? 1 : 0};
        }
        hipStream_t st = P->ctx->stream;
        // the scratch: 2 x (w + 2 L - 2) int32 per range, less what lies below base 0; out of memory is the plan's refusal
        HIP_TRY(P->pool.alloc(&Q.scratch, (size_t)std::max<int64_t>(P->off.back(), 1)));
        HIP_TRY(P->pool.alloc(&Q.ranges, (size_t)std::max<int64_t>(n, 1)));
        if (n) HIP_TRY(hipMemcpyAsync(Q.ranges, rg.data(), rg.size() * sizeof(BsigCappedRange), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const auto form = [&](bool wide) {
        return bsig::capped_form(P->threads, P->kp.packed_half != 0, wide, !cover && Q.binned, P->tile_cells, cover ? 2 : Q.S, Q.n_acc);
    };
    const size_t lds = form(n_wide > 0).lds;
    const auto refuse = [&](int lds_max) {
        return fail(BSIG_ERR_ARG, "a tile of %d cells and its bins need %zu bytes of LDS per workgroup, the device has %d", P->tile_cells, lds,
                    lds_max);
    };
    return setup_runs(P, lds, refuse, form(false), "BAMSIGNALS_CAPPED_RUN_TILES", kCounterMax,
                      [&](int64_t t) { return (int64_t)items[(size_t)t].nc; }, n_wide);
}

extern "C" {

int bsig_plan_create(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid,
                     const int32_t *loc, const int32_t *len, const int32_t *strand,
                     const bsig_params *prm, bsig_plan **out)
{
    return plan_create_impl(ctx, reads, n, rid, loc, len, strand, prm, PlanRequest{}, out);
}

// A resized plan is an ORDINARY plan whose reads cover frag_len bases from their 5' end (kernels.hip: covered_interval):
// only the rule's frag_len and the window's ext differ.  The packed class takes every sum from its chunk's base, which
// lies within ext + maxspan + a bucket of the tile: with frag_len <= BSIG_FRAG_LEN_MAX = 2^24 all of them stay below 2^26.
int bsig_plan_create_resized(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid,
                             const int32_t *loc, const int32_t *len, const int32_t *strand,
                             const bsig_params *prm, int32_t frag_len, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_resized");
    *out = nullptr;
    if (const int rc = bsig::resized_rule(*prm, frag_len)) return rc;
    PlanRequest rq;
    rq.frag_len = frag_len;
    return plan_create_impl(ctx, reads, n, rid, loc, len, strand, prm, rq, out);
}

// (a capped coverage plan's own layout is its scratch's: the caller sees the result's)
static const std::vector<int64_t> &result_layout(const bsig_plan *p)
{
    return p->red && !p->red->capped.res_off.empty() ? p->red->capped.res_off : p->off;
}
const int64_t *bsig_plan_offsets(const bsig_plan *p) { return p ? result_layout(p).data() : nullptr; }

int64_t bsig_plan_cells(const bsig_plan *p) { return p ? result_layout(p).back() : 0; }

}  // extern "C"
// The main launch of a run, bsig_plan_run's or bsig_plan_run_sum's: launch(kp, resolved, lookup) enqueues it in the form
// chosen here.  Large launches look their tiles' windows up in a launch of their own (k_resolve_tiles, one lane per
// tile), so that a pileup workgroup -- which holds its LDS and registers from its first instruction on -- gets its work
// item and its windows in ONE memory round trip instead of two dependent ones; small launches, where a second launch
// costs more than it hides, look them up inside the pileup kernel (bam_itr_queryi's counterpart, ref: :267).  A plan and
// a layout of the reads are both immutable, so the windows are a function of the two: the lookup launch runs in the
// plan's FIRST run on a layout and its result is kept with the plan (round 5; 9-11 us of every later step of a resident
// plan; env BAMSIGNALS_CACHE_WINDOWS=0: looked up in every run, as in round 4).  A file-level call makes its plan and
// runs it once: it looks its windows up once either way.
template <typename Launch>
static int run_main(bsig_plan *p, Launch &&launch)
{
    if (!plan_two_launches(p)) {
        HIP_TRY(launch(p->kp, nullptr, false));
        return BSIG_OK;
    }
    const bool lookup = !windows_kept() || p->resolved_gen != p->reads->layout_gen;
    if (!p->resolved) HIP_TRY(p->pool.alloc(&p->resolved, (size_t)p->n_items));
    BsigKParams res = p->kp;
    res.resolved = 1;
    HIP_TRY(launch(res, p->resolved, lookup));
    p->resolved_gen = p->reads->layout_gen;
    return BSIG_OK;
}
// The one refusal of a run call of kind `want` for a plan of another kind (BSIG_OK: it is that kind).  A plan of a later
// kind is told which call runs it, one of an earlier kind what it is not; host: the entry is a _host one, so the call named
// is too (bsig_plan_run_host_async names the device calls).
static int wrong_kind(const bsig_plan *p, PlanKind want, bool host)
{
    if (p->kind == want) return BSIG_OK;
    const char *call = host ? kKinds[p->kind].run_host : kKinds[p->kind].run_dev;
    if (p->kind > want) return fail(BSIG_ERR_ARG, "%s plan runs with %s", kKinds[p->kind].a, call);
    return fail(BSIG_ERR_ARG, "not %s plan: %s runs it", kKinds[want].a, call);
}
// What the device run calls of every kind but kPlain do around their launches: the checks in the order every one of them made them, the
// plan's GPU made current, then body(the plan's Reduced, its stream) -- the launches -- and the run counted.
template <typename Body>
static int run_reduced(bsig_plan *p, PlanKind want, void *dev, Body &&body)
{
    if (!p) return fail(BSIG_ERR_ARG, "plan is NULL");
    if (const int rc = wrong_kind(p, want, false)) return rc;
    if (p->red->cells == 0) return BSIG_OK;      // (a sum or a V-plot over ranges without width: the other kinds always have cells)
    if (!dev) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    if (((uintptr_t)dev & 7) != 0) return fail(BSIG_ERR_ARG, "device output buffer must be 8-byte aligned");
    if (p->reads->layout_gen != p->made_for_gen)
        return fail(BSIG_ERR_ARG, "the reads were laid out again after this plan was made: make a new plan");
    HIP_TRY(hipSetDevice(p->ctx->device));      // the caller's thread may have another GPU current
    if (const int rc = body(*p->red, p->ctx->stream)) return rc;
    ++p->runs;
    return BSIG_OK;
}
// The body of the run calls whose kernels ADD into the result (xcorr, frag, hist, summary, scaled): the result zeroed, the
// main launch in the form run_main chose, then the extra runs -- the tiles with more reads than a 16-bit cell may see: whole,
// with 32-bit cells, their windows looked up in place.  launch(wide, kp, items, n_items, runs, n_runs, windows, lookup) is the
// kind's launch_*_tiles.  zero false: every cell is stored by the tile that owns it (a capped plan with bins of one base).
template <typename Launch>
static int run_added(bsig_plan *p, const Reduced &R, void *dev, hipStream_t st, Launch &&launch, bool zero = true)
{
    if (zero) HIP_TRY(hipMemsetAsync(dev, 0, (size_t)R.cells * (size_t)kKinds[p->kind].cell_bytes, st));
    if (R.n_runs_main) {
        const int rc = run_main(p, [&](const BsigKParams &kp, BsigResolved *resolved, bool lookup) {
            return launch(false, kp, p->items, p->n_items, R.runs, R.n_runs_main, resolved, lookup);
        });
        if (rc != BSIG_OK) return rc;
    }
    if (R.n_runs_extra)
        HIP_TRY(launch(true, p->kp, p->heavy_items, p->n_heavy_slices, R.runs + R.n_runs_main, R.n_runs_extra, nullptr, false));
    return BSIG_OK;
}
extern "C" {

int bsig_plan_run(bsig_plan *p, int32_t *out_dev)
{
    if (!p) return fail(BSIG_ERR_ARG, "plan is NULL");
    if (const int rc = wrong_kind(p, kPlain, false)) return rc;
    const int64_t cells = p->off.back();
    if (cells == 0) return BSIG_OK;
    if (!out_dev) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    if (((uintptr_t)out_dev & 15) != 0) return fail(BSIG_ERR_ARG, "device output buffer must be 16-byte aligned");
    if (p->reads->layout_gen != p->made_for_gen)
        return fail(BSIG_ERR_ARG, "the reads were laid out again after this plan was made: make a new plan");
    HIP_TRY(hipSetDevice(p->ctx->device));      // the caller's thread may have another GPU current
    hipStream_t st = p->ctx->stream;
    // (heavy tiles need no fill: their main item stores 0 and only the slices add)
    if (p->kernel_mode == BSIG_MODE_COUNT && p->needs_zero)
        HIP_TRY(hipMemsetAsync(out_dev, 0, cells * sizeof(int32_t), st));
    const int rc = run_main(p, [&](const BsigKParams &kp, BsigResolved *resolved, bool lookup) {
        return bsig::launch_pileup(p->kernel_mode, p->kp.ss, p->threads, p->reads->dev, kp, p->items, p->n_items, p->tile_cells,
                                   resolved, lookup, out_dev, st);
    });
    if (rc != BSIG_OK) return rc;
    if (p->n_heavy_slices) {
        // the first launch zero-filled the heavy tiles; their slices now add their partial images
        if (p->overflow) HIP_TRY(hipMemsetAsync(p->overflow, 0, sizeof(int32_t), st));     // (the flag speaks of this run)
        BsigKParams acc = p->kp;
        acc.accumulate = 1;
        HIP_TRY(bsig::launch_pileup(p->kernel_mode, p->kp.ss, p->threads, p->reads->dev, acc, p->heavy_items,
                                    p->n_heavy_slices, p->tile_cells, p->heavy_windows, false, out_dev, st));
    }
    ++p->runs;
    return BSIG_OK;
}

int bsig_plan_run_host(bsig_plan *p, int32_t *out_host)
{
    if (!p) return fail(BSIG_ERR_ARG, "plan is NULL");
    if (const int rc = wrong_kind(p, kPlain, true)) return rc;
    const bsig::HostDest dst{out_host};
    return bsig::plan_run_to_host(p, &dst);
}

int bsig_plan_overflowed(bsig_plan *p, int32_t *flag)
{
    if (!p || !flag) return fail(BSIG_ERR_ARG, "NULL argument");
    *flag = 0;
    if (!p->overflow || !p->runs) return BSIG_OK;
    HIP_TRY(hipSetDevice(p->ctx->device));
    HIP_TRY(hipMemcpyAsync(flag, p->overflow, sizeof(int32_t), hipMemcpyDeviceToHost, p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return BSIG_OK;
}

}  // extern "C"
int bsig::plan_run_to_host(bsig_plan *p, const HostDest *dst, bool async, double *t_kernels, double *t_download)
{
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
    const int64_t cells = p->off.back();
    if (cells == 0) return BSIG_OK;
    if (!dst || (!dst->flat && !dst->ptrs)) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    HIP_TRY(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    if (!p->d_out) HIP_TRY(p->pool.alloc(&p->d_out, (size_t)cells));
    int rc = bsig_plan_run(p, p->d_out);
    if (rc != BSIG_OK) return rc;
    if (t_kernels) {
        HIP_TRY(hipStreamSynchronize(st));
        *t_kernels = since(t0);
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (async) {
        HIP_TRY(hipMemcpyAsync(dst->flat, p->d_out, (size_t)cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return BSIG_OK;
    }
    rc = download_to_dest(p->ctx, p->d_out, *dst, cells);
    if (t_download) *t_download = since(t1);
    return rc != BSIG_OK ? rc : plan_check_overflow(p);
}
int bsig::plan_run_reduced_to_host(bsig_plan *p, void *host, double *t_kernels, double *t_download)
{
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
    Reduced *Q = p->red.get();
    if (!Q) return fail(BSIG_ERR_ARG, "not a reduction plan: %s runs it", kKinds[kPlain].run_host);
    if (Q->cells == 0) return BSIG_OK;
    if (!host) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    HIP_TRY(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    const size_t bytes = (size_t)Q->cells * (size_t)kKinds[p->kind].cell_bytes;
    if (!Q->d_out) HIP_TRY(p->pool.alloc(&Q->d_out, (bytes + 7) / 8));
    int rc = BSIG_OK;
    switch (p->kind) {
    case kPlain: break;
    case kSum: rc = bsig_plan_run_sum(p, Q->d_out); break;
    case kXcorr: rc = bsig_plan_run_xcorr(p, Q->d_out); break;
    case kFrag: rc = bsig_plan_run_frag(p, Q->d_out); break;
    case kHist: rc = bsig_plan_run_hist(p, Q->d_out); break;
    case kSummary: rc = bsig_plan_run_summary(p, Q->d_out); break;
    case kScaled: rc = bsig_plan_run_scaled(p, Q->d_out); break;
    case kVplot: rc = bsig_plan_run_vplot(p, Q->d_out); break;
    case kCapped: rc = bsig_plan_run_capped(p, reinterpret_cast<int32_t *>(Q->d_out)); break;
    }
    if (rc != BSIG_OK) return rc;
    if (t_kernels) {
        HIP_TRY(hipStreamSynchronize(st));
        *t_kernels = since(t0);
    }
    const auto t1 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(host, Q->d_out, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (t_download) *t_download = since(t1);
    return BSIG_OK;
}
// a run whose slices took a bin past INT32_MAX fails (after the caller's synchronisation: no wait of its own)
int bsig::plan_check_overflow(bsig_plan *p)
{
    int32_t f = 0;
    const int rc = bsig_plan_overflowed(p, &f);
    if (rc != BSIG_OK) return rc;
    if (f) return fail(BSIG_ERR_ARG, "a coverage bin exceeds 2^31 - 1 reads x bases: choose a smaller binsize");
    return BSIG_OK;
}
extern "C" {

int bsig_plan_run_host_async(bsig_plan *p, int32_t *out_host)
{
    if (!p) return fail(BSIG_ERR_ARG, "plan is NULL");
    if (const int rc = wrong_kind(p, kPlain, false)) return rc;
    const bsig::HostDest dst{out_host};
    return bsig::plan_run_to_host(p, &dst, true);
}

// The visit counts are taken once (a launch of k_visits); what follows from them is worked out at every call from the
// plan's state, so that it describes the form the plan's next run takes.
int bsig_plan_get_stats(bsig_plan *p, bsig_plan_stats *s)
{
    if (!p || !s) return fail(BSIG_ERR_ARG, "NULL argument");
    const unsigned long long *acc = p->visits;
    if (!p->have_visits) {
        hipStream_t st = p->ctx->stream;
        unsigned long long *d_acc = nullptr;
        HIP_TRY(hipSetDevice(p->ctx->device));
        HIP_TRY(hipMalloc((void **)&d_acc, sizeof p->visits));
        hipError_t e = hipMemsetAsync(d_acc, 0, sizeof p->visits, st);
        if (e == hipSuccess) e = bsig::launch_visits(p->reads->dev, p->kp, p->kernel_mode, p->items, p->n_items, d_acc, st);
        if (e == hipSuccess) e = hipMemcpyAsync(p->visits, d_acc, sizeof p->visits, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(d_acc);
        if (e != hipSuccess) return fail(BSIG_ERR_DEVICE, "visit count failed: %s", hipGetErrorString(e));
        p->have_visits = true;
    }
    bsig_plan_stats t{};
    t.n_ranges = p->n_ranges;
    t.n_items = p->n_items;
    t.cells = p->red ? p->red->cells : p->off.back();
    t.visits_packed = (int64_t)acc[BSIG_CLASS_PACKED];   // one word per read
    t.visits_short = (int64_t)(acc[0] + acc[1]);         // classes 0 and 1: no end column
    t.visits = (int64_t)(acc[0] + acc[1] + acc[2] + acc[3] + acc[BSIG_CLASS_PACKED]);
    t.streamed = (int64_t)acc[BSIG_MAX_CLASSES];
    t.heavy_tiles = (int32_t)std::min<int64_t>(p->n_heavy_tiles, INT32_MAX);
    t.bytes_per_visit_packed = p->kp.packed_half ? 2 : p->kp.use_tlen ? 8 : 4;     // the half-word, or the packed word [+ tlen]
    // span <= 4096: the half-word, or pos + flag/mapq/span in one word [+ tlen]
    t.bytes_per_visit_short = p->kp.short_half ? 2 : p->kp.use_tlen ? 12 : 8;
    t.bytes_per_visit_long = p->kp.use_tlen ? 16 : 12;     // pos + end + flag/mapq [+ tlen]
    // reads + work items + index entries + result cells (a sum plan: 8 B a cell of the sum, none per range)
    const int64_t per_item = (int64_t)sizeof(BsigWorkItem);
    t.algorithmic_bytes = t.bytes_per_visit_packed * t.visits_packed + t.bytes_per_visit_short * t.visits_short +
                          t.bytes_per_visit_long * (t.visits - t.visits_short - t.visits_packed) + per_item * t.n_items +
                          kKinds[p->kind].cell_bytes * t.cells;
    if (plan_two_launches(p) && windows_kept()) {
        // a resident plan's step reads the windows kept from its first run: no index entry is touched
        t.algorithmic_bytes += (int64_t)sizeof(BsigResolved) * t.n_items;
    } else {
        t.algorithmic_bytes += 8 * t.n_items * p->reads->info.n_classes;          // the index entries
        // two launches: the work item is read twice and the tile's windows are written and read once
        if (plan_two_launches(p)) t.algorithmic_bytes += (per_item + 2 * (int64_t)sizeof(BsigResolved)) * t.n_items;
    }
    *s = t;
    return BSIG_OK;
}

void bsig_plan_free(bsig_plan *p) { delete p; }

// bsig_plan_create_sum (frag_len 0) and bsig_plan_create_sum_resized (frag_len judged by resized_rule)
static int plan_create_sum_impl(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                                const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t frag_len, bsig_plan **out)
{
    if (n < 0 || (n > 0 && !len)) return fail(BSIG_ERR_ARG, "range arrays missing");
    bsig::SumShape shape;
    bsig::PlanRule caller;          // (the caller's binsize and threads; the per-base tiles' are the plan's)
    int rc = bsig::sum_shape(*prm, n, len, &shape);
    if (rc == BSIG_OK) rc = bsig::check_params(*prm, n, len, &caller, frag_len);
    PlanRequest rq;
    rq.kind = kSum;
    rq.frag_len = frag_len;
    rq.sum = &shape;
    return rc != BSIG_OK ? rc : plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
}

int bsig_plan_create_sum(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                         const int32_t *len, const int32_t *strand, const bsig_params *prm, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_sum");
    *out = nullptr;
    return plan_create_sum_impl(ctx, reads, n, rid, loc, len, strand, prm, 0, out);
}

int bsig_plan_create_sum_resized(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                                 const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t frag_len,
                                 bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_sum_resized");
    *out = nullptr;
    if (const int rc = bsig::resized_rule(*prm, frag_len)) return rc;
    return plan_create_sum_impl(ctx, reads, n, rid, loc, len, strand, prm, frag_len, out);
}

int bsig_plan_create_xcorr(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                           const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t max_lag, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_xcorr");
    *out = nullptr;
    bsig::XcorrShape shape;
    const int rc = bsig::xcorr_shape(*prm, max_lag, &shape);
    PlanRequest rq;
    rq.kind = kXcorr;
    rq.xcorr = &shape;
    return rc != BSIG_OK ? rc : plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
}

int bsig_plan_create_frag(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                          const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t len_bin, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_frag");
    *out = nullptr;
    bsig::FragShape shape;
    const int rc = bsig::frag_shape(*prm, len_bin, &shape);
    PlanRequest rq;
    rq.kind = kFrag;
    rq.frag = &shape;
    return rc != BSIG_OK ? rc : plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
}

int bsig_plan_create_hist(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                          const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t max_value, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_hist");
    *out = nullptr;
    bsig::HistShape shape;
    const int rc = bsig::hist_shape(*prm, max_value, &shape);
    PlanRequest rq;
    rq.kind = kHist;
    rq.hist = &shape;
    return rc != BSIG_OK ? rc : plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
}

int bsig_plan_create_summary(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                             const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t n_thresholds,
                             const int32_t *thresholds, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_summary");
    *out = nullptr;
    bsig::SummaryShape shape;
    const int rc = bsig::summary_shape(*prm, n_thresholds, thresholds, &shape);
    PlanRequest rq;
    rq.kind = kSummary;
    rq.summary = &shape;
    return rc != BSIG_OK ? rc : plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
}

int bsig_plan_create_scaled(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                            const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t n_bins, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_scaled");
    *out = nullptr;
    bsig::ScaledShape shape;
    const int rc = bsig::scaled_shape(*prm, n_bins, &shape);
    PlanRequest rq;
    rq.kind = kScaled;
    rq.scaled = &shape;
    return rc != BSIG_OK ? rc : plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
}

int bsig_plan_create_capped(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                            const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t keep_dup, int32_t frag_len,
                            bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_capped");
    *out = nullptr;
    bsig::CappedShape shape;
    if (const int rc = bsig::capped_shape(*prm, keep_dup, frag_len, &shape)) return rc;
    PlanRequest rq;
    rq.kind = kCapped;
    rq.capped = &shape;
    if (!frag_len) return plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
    // the capped coverage: stage 1 walks the widened ranges, every one as a '+' range (the scratch is in genome order)
    if (n < 0 || (n > 0 && (!rid || !loc || !len || !strand))) return fail(BSIG_ERR_ARG, "range arrays missing");
    std::vector<int32_t> wloc((size_t)n), wlen((size_t)n), lead((size_t)n), plus((size_t)n, 1);
    for (int64_t i = 0; i < n; ++i) {
        if (len[i] < 0) return fail(BSIG_ERR_ARG, "range %lld has a negative width", (long long)i);
        const bsig::CappedWide c = bsig::capped_widen(loc[i], len[i], frag_len);
        if (!c.fits)
            return fail(BSIG_ERR_ARG, "range %lld widened by the fragment length ends beyond 2^31 - 1: cut the range", (long long)i);
        wloc[(size_t)i] = c.loc; wlen[(size_t)i] = c.len; lead[(size_t)i] = c.lead;
    }
    shape.len0 = len; shape.strand0 = strand; shape.lead = lead.data();
    return plan_create_impl(ctx, reads, n, rid, wloc.data(), wlen.data(), plus.data(), &shape.tiles, rq, out);
}

int bsig_plan_create_vplot(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc,
                           const int32_t *len, const int32_t *strand, const bsig_params *prm, int32_t len_bin, bsig_plan **out)
{
    if (!ctx || !reads || !prm || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_plan_create_vplot");
    *out = nullptr;
    if (n < 0 || (n > 0 && !len)) return fail(BSIG_ERR_ARG, "range arrays missing");
    bsig::VplotShape shape;
    const int rc = bsig::vplot_shape(*prm, n, len, len_bin, &shape);
    PlanRequest rq;
    rq.kind = kVplot;
    rq.vplot = &shape;
    return rc != BSIG_OK ? rc : plan_create_impl(ctx, reads, n, rid, loc, len, strand, &shape.tiles, rq, out);
}

// a kind's queries answer 0 for a plan of another kind (and for no plan)
static int64_t cells_if(const bsig_plan *p, PlanKind kind) { return p && p->kind == kind ? p->red->cells : 0; }
static int64_t runs_if(const bsig_plan *p, PlanKind kind) { return p && p->kind == kind ? p->red->n_runs_main + p->red->n_runs_extra : 0; }
int64_t bsig_plan_sum_cells(const bsig_plan *p) { return cells_if(p, kSum); }
int64_t bsig_plan_xcorr_cells(const bsig_plan *p) { return cells_if(p, kXcorr); }
int64_t bsig_plan_frag_cells(const bsig_plan *p) { return cells_if(p, kFrag); }
int64_t bsig_plan_frag_runs(const bsig_plan *p) { return runs_if(p, kFrag); }
int64_t bsig_plan_hist_cells(const bsig_plan *p) { return cells_if(p, kHist); }
int64_t bsig_plan_hist_runs(const bsig_plan *p) { return runs_if(p, kHist); }
int64_t bsig_plan_summary_cells(const bsig_plan *p) { return cells_if(p, kSummary); }
int64_t bsig_plan_summary_runs(const bsig_plan *p) { return runs_if(p, kSummary); }
int64_t bsig_plan_scaled_cells(const bsig_plan *p) { return cells_if(p, kScaled); }
int64_t bsig_plan_scaled_runs(const bsig_plan *p) { return runs_if(p, kScaled); }
int32_t bsig_plan_scaled_segmented(const bsig_plan *p) { return p && p->kind == kScaled && p->red->scaled.segmented ? 1 : 0; }
int64_t bsig_plan_vplot_cells(const bsig_plan *p) { return cells_if(p, kVplot); }
int64_t bsig_plan_vplot_runs(const bsig_plan *p) { return runs_if(p, kVplot); }
int32_t bsig_plan_vplot_rows(const bsig_plan *p) { return p && p->kind == kVplot ? p->red->vplot.rows : 0; }
int32_t bsig_plan_vplot_cols(const bsig_plan *p) { return p && p->kind == kVplot ? p->red->vplot.cols : 0; }
int32_t bsig_plan_vplot_form(const bsig_plan *p) { return p && p->kind == kVplot ? p->red->vplot.form : 0; }
int64_t bsig_plan_capped_cells(const bsig_plan *p) { return cells_if(p, kCapped); }
int64_t bsig_plan_capped_runs(const bsig_plan *p) { return runs_if(p, kCapped); }

int bsig_plan_run_sum(bsig_plan *p, int64_t *sum_dev)
{
    return run_reduced(p, kSum, sum_dev, [&](const Reduced &R, hipStream_t st) -> int {
        const auto &Q = R.sum;
        const int ss = Q.S == 2, nw = Q.nw;
        if (R.n_runs_main) {
            const int rc = run_main(p, [&](const BsigKParams &kp, BsigResolved *resolved, bool lookup) {
                return bsig::launch_sum_tiles(Q.kind, ss, nw, p->reads->dev, kp, p->items, p->n_items, R.runs, R.n_runs_main,
                                              resolved, lookup, Q.slab, st);
            });
            if (rc != BSIG_OK) return rc;
        }
        // the slices of heavy tiles: one more addend each, with their fixed windows, into slabs of their own
        if (R.n_runs_extra)
            HIP_TRY(bsig::launch_sum_tiles(Q.kind, ss, nw, p->reads->dev, p->kp, p->heavy_items, p->n_heavy_slices,
                                           R.runs + R.n_runs_main, R.n_runs_extra, p->heavy_windows, false,
                                           Q.slab + (size_t)R.n_runs_main * (size_t)Q.slab_vals, st));
        const int32_t width = Q.width, binsize = Q.binsize;
        long long *base = binsize == 1 ? reinterpret_cast<long long *>(sum_dev) : Q.base;
        HIP_TRY(hipMemsetAsync(base, 0, (size_t)width * Q.S * sizeof(long long), st));
        HIP_TRY(bsig::launch_sum_reduce(Q.kind != kSumProfile, Q.slab, Q.slab_vals, Q.chunks, Q.n_chunks, Q.max_nvals,
                                        reinterpret_cast<unsigned long long *>(base), st));
        if (Q.kind != kSumProfile) HIP_TRY(bsig::launch_sum_scan(base, width, p->tile_cells, Q.S, st));
        if (binsize != 1) HIP_TRY(bsig::launch_sum_bins(base, width, binsize, Q.S, R.cells, reinterpret_cast<long long *>(sum_dev), st));
        return BSIG_OK;
    });
}

int bsig_plan_run_xcorr(bsig_plan *p, int64_t *dev)
{
    return run_reduced(p, kXcorr, dev, [&](const Reduced &R, hipStream_t st) -> int {
        // (moments[0], the ranges' cells, is the main launch's first workgroup's to add: ranges with cells have tiles)
        return run_added(p, R, dev, st, [&](bool wide, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items, const uint2 *runs,
                                            int64_t n_runs, void *windows, bool lookup) {
            return bsig::launch_xcorr_tiles(p->threads, wide, p->reads->dev, kp, items, n_items, runs, n_runs, windows, lookup, R.xcorr.body,
                                            R.xcorr.max_lag, wide ? 0ull : (unsigned long long)R.xcorr.n_cells,
                                            reinterpret_cast<unsigned long long *>(dev), st);
        });
    });
}

int bsig_plan_run_frag(bsig_plan *p, int64_t *dev)
{
    return run_reduced(p, kFrag, dev, [&](const Reduced &R, hipStream_t st) -> int {
        return run_added(p, R, dev, st, [&](bool, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items, const uint2 *runs,
                                            int64_t n_runs, void *windows, bool lookup) {
            return bsig::launch_frag_tiles(p->threads, R.frag.merge, p->reads->dev, kp, items, n_items, runs, n_runs, windows, lookup,
                                           (int)R.cells, R.frag.len_bin, reinterpret_cast<unsigned long long *>(dev), st);
        });
    });
}

int bsig_plan_run_hist(bsig_plan *p, int64_t *dev)
{
    return run_reduced(p, kHist, dev, [&](const Reduced &R, hipStream_t st) -> int {
        const auto &Q = R.hist;
        // (moments[0], the ranges' cells, is the main launch's first workgroup's to add: ranges with cells have tiles)
        return run_added(p, R, dev, st, [&](bool wide, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items, const uint2 *runs,
                                            int64_t n_runs, void *windows, bool lookup) {
            return bsig::launch_hist_tiles(p->threads, Q.coverage, wide, Q.merge, p->reads->dev, kp, items, n_items, runs, n_runs, windows,
                                           lookup, Q.max_value + 1, wide ? 0ull : (unsigned long long)Q.n_cells,
                                           reinterpret_cast<unsigned long long *>(dev), st);
        });
    });
}

int bsig_plan_run_summary(bsig_plan *p, int64_t *dev)
{
    return run_reduced(p, kSummary, dev, [&](const Reduced &R, hipStream_t st) -> int {
        const auto &Q = R.summary;
        const int rc = run_added(p, R, dev, st, [&](bool wide, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items,
                                                    const uint2 *runs, int64_t n_runs, void *windows, bool lookup) {
            return bsig::launch_summary_tiles(p->threads, Q.coverage, wide, p->reads->dev, kp, items, n_items, runs, n_runs, windows, lookup,
                                              Q.thr, reinterpret_cast<unsigned long long *>(dev), st);
        });
        if (rc != BSIG_OK) return rc;
        // every row's key into its max and summit (rows no tile wrote -- ranges without width -- get summit -1)
        HIP_TRY(bsig::launch_summary_finish(p->n_ranges * Q.S, BSIG_SUMMARY_FIXED + Q.thr.k, reinterpret_cast<long long *>(dev), st));
        return BSIG_OK;
    });
}

int bsig_plan_run_scaled(bsig_plan *p, int64_t *dev)
{
    return run_reduced(p, kScaled, dev, [&](const Reduced &R, hipStream_t st) -> int {
        const auto &Q = R.scaled;
        return run_added(p, R, dev, st, [&](bool wide, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items, const uint2 *runs,
                                            int64_t n_runs, void *windows, bool lookup) {
            return bsig::launch_scaled_tiles(p->threads, Q.coverage, wide, Q.segmented, p->reads->dev, kp, items, n_items, runs, n_runs,
                                             windows, lookup, Q.n_bins, reinterpret_cast<unsigned long long *>(dev), st);
        });
    });
}

int bsig_plan_run_vplot(bsig_plan *p, int64_t *dev)
{
    return run_reduced(p, kVplot, dev, [&](const Reduced &R, hipStream_t st) -> int {
        const auto &Q = R.vplot;
        return run_added(p, R, dev, st, [&](bool, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items, const uint2 *runs,
                                            int64_t n_runs, void *windows, bool lookup) {
            return bsig::launch_vplot_tiles(p->threads, Q.form != 0, Q.merge, Q.lds_budget, p->reads->dev, kp, items, n_items, runs, n_runs, windows,
                                            lookup, Q.rows, Q.cols, Q.len_bin, Q.binsize, Q.bin_magic, Q.bin_shift,
                                            reinterpret_cast<unsigned long long *>(dev), st);
        });
    });
}

int bsig_plan_run_capped(bsig_plan *p, int32_t *dev)
{
    return run_reduced(p, kCapped, dev, [&](const Reduced &R, hipStream_t st) -> int {
        const auto &Q = R.capped;
        if (!Q.frag_len)
            return run_added(p, R, dev, st, [&](bool wide, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items,
                                                const uint2 *runs, int64_t n_runs, void *windows, bool lookup) {
                return bsig::launch_capped_tiles(p->threads, wide, Q.binned, p->reads->dev, kp, items, n_items, runs, n_runs, windows,
                                                 lookup, Q.keep_dup, Q.S == 2, Q.bin_magic, Q.bin_shift, Q.n_acc, dev, st);
            }, Q.binned);
        // the capped coverage: the capped ends of the widened ranges into the scratch (every pair has its tile: nothing to
        // zero), its rows' prefix sums, then the window sums into the result
        int32_t *scratch = reinterpret_cast<int32_t *>(Q.scratch);
        const int rc = run_added(p, R, scratch, st, [&](bool wide, const BsigKParams &kp, const BsigWorkItem *items, int64_t n_items,
                                                        const uint2 *runs, int64_t n_runs, void *windows, bool lookup) {
            return bsig::launch_capped_tiles(p->threads, wide, false, p->reads->dev, kp, items, n_items, runs, n_runs, windows, lookup,
                                             Q.keep_dup, 1, 0u, 0, 0, scratch, st);
        }, false);
        if (rc != BSIG_OK) return rc;
        HIP_TRY(bsig::launch_capped_scan(Q.ranges, p->n_ranges, Q.scratch, st));
        if (Q.binned) HIP_TRY(hipMemsetAsync(dev, 0, (size_t)R.cells * sizeof(int32_t), st));
        HIP_TRY(bsig::launch_capped_cover(Q.ranges, p->n_ranges, Q.scratch, Q.frag_len, Q.S == 2, Q.binned, Q.bin_magic, Q.bin_shift, dev, st));
        return BSIG_OK;
    });
}

// the _host calls: the kind checked, then the one run into the plan's own device buffer and its download
static int run_reduced_host(bsig_plan *p, PlanKind want, void *host)
{
    if (!p) return fail(BSIG_ERR_ARG, "plan is NULL");
    if (const int rc = wrong_kind(p, want, true)) return rc;
    return bsig::plan_run_reduced_to_host(p, host);
}
int bsig_plan_run_sum_host(bsig_plan *p, int64_t *sum_host) { return run_reduced_host(p, kSum, sum_host); }
int bsig_plan_run_xcorr_host(bsig_plan *p, int64_t *host) { return run_reduced_host(p, kXcorr, host); }
int bsig_plan_run_frag_host(bsig_plan *p, int64_t *host) { return run_reduced_host(p, kFrag, host); }
int bsig_plan_run_hist_host(bsig_plan *p, int64_t *host) { return run_reduced_host(p, kHist, host); }
int bsig_plan_run_summary_host(bsig_plan *p, int64_t *host) { return run_reduced_host(p, kSummary, host); }
int bsig_plan_run_scaled_host(bsig_plan *p, int64_t *host) { return run_reduced_host(p, kScaled, host); }
int bsig_plan_run_vplot_host(bsig_plan *p, int64_t *host) { return run_reduced_host(p, kVplot, host); }
int bsig_plan_run_capped_host(bsig_plan *p, int32_t *host) { return run_reduced_host(p, kCapped, host); }

// (tests: what a re-layout of the resident columns does to the plans made before it)
// The segment table of a plan's own layout, for the encoders of a per-range result (runs.hip, views.hip): range i's cells
// off[i] .. off[i + 1] are one segment, or with strands the two rows of the 2 * bin + antisense cells (stride 2)
static int plan_segments(const bsig_plan *p, const char *what, std::vector<int64_t> &base, std::vector<int32_t> &len, int *stride)
{
    if (p->kind != kPlain)      // (the kind's noun without its article)
        return fail(BSIG_ERR_ARG, "a %s plan has no per-range result to encode", strchr(kKinds[p->kind].a, ' ') + 1);
    if (p->mode == BSIG_MODE_COUNT) return fail(BSIG_ERR_ARG, "bamCount has no %s: one cell per range", what);
    const int S = p->kp.ss ? 2 : 1;
    base.resize((size_t)(p->n_ranges * S));
    len.resize((size_t)(p->n_ranges * S));
    for (int64_t i = 0; i < p->n_ranges; ++i)
        for (int a = 0; a < S; ++a) {
            base[(size_t)(i * S + a)] = p->off[(size_t)i] + a;
            len[(size_t)(i * S + a)] = (int32_t)((p->off[(size_t)i + 1] - p->off[(size_t)i]) / S);
        }
    *stride = S;
    return BSIG_OK;
}

int bsig_plan_runs_create(const bsig_plan *p, bsig_runs **out)
{
    if (!p || !out) return fail(BSIG_ERR_ARG, "NULL argument");
    *out = nullptr;
    std::vector<int64_t> base;
    std::vector<int32_t> len;
    int S = 1;
    if (const int rc = plan_segments(p, "runs", base, len, &S)) return rc;
    return bsig_runs_create(p->ctx, p->n_ranges * S, base.data(), len.data(), S, out);
}

int bsig_plan_views_create(const bsig_plan *p, bsig_views **out)
{
    if (!p || !out) return fail(BSIG_ERR_ARG, "NULL argument");
    *out = nullptr;
    std::vector<int64_t> base;
    std::vector<int32_t> len;
    int S = 1;
    if (const int rc = plan_segments(p, "views", base, len, &S)) return rc;
    return bsig_views_create(p->ctx, p->n_ranges * S, base.data(), len.data(), S, out);
}

int bsig_debug_new_layout_gen(bsig_reads *reads)
{
    if (!reads) return 1;
    reads->layout_gen = bsig::next_layout_gen();
    return 0;
}

int bsig_debug_set_resolve_min(long long n_tiles)
{
    g_resolve_min_override = n_tiles;
    return 0;
}

int bsig_pileup_columns(bsig_ctx *ctx, const bsig_reads *reads, int64_t n, const int32_t *rid,
                        const int32_t *loc, const int32_t *len, const int32_t *strand,
                        const bsig_params *params, int32_t *out_host, const int64_t *off)
{
    bsig_plan *p = nullptr;
    int rc = bsig_plan_create(ctx, reads, n, rid, loc, len, strand, params, &p);
    if (rc != BSIG_OK) return rc;
    if (off && memcmp(off, p->off.data(), (n + 1) * sizeof(int64_t)) != 0) {
        bsig_plan_free(p);
        return fail(BSIG_ERR_ARG, "offsets do not match bsig_layout() for these parameters");
    }
    rc = bsig_plan_run_host(p, out_host);
    bsig_plan_free(p);
    return rc;
}

}  // extern "C"
