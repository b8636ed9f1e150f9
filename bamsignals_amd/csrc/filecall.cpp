// The file-level dispatcher: every bsig_pileup_* / bsig_coverage_* / bsig_overlap_core entry point (fileapi.cpp) comes
// through file_level() below, a short sequence of stages -- judge the call, open the BAM, resolve the ranges, find the GPUs,
// acquire the reads, run the result.  Also here: what the calls keep between calls (the cache) and the multi-GPU result
// routes.  Pure host code; the compute goes through bsig_reads_* / bsig_plan_*.
#include "filecall.h"

#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>

#include "collect.h"
#include "genecounts.h"
#include "host_util.h"
#include "junctions.h"
#include "nucleotides.h"
#include "sites.h"
#include "rangemath.h"

namespace bsig {
namespace {

// stage seconds of the calling thread's last file-level call: open (header + BAI), decode,
// upload + HBM layout, plan + kernels + result download, total; [5] = 1 if the BAM was already
// resident in HBM
thread_local double g_call_timing[6] = {0, 0, 0, 0, 0, 0};
// ... and where the time of its stages went (bsig_last_call_timing_ex, slots 6..15)
thread_local double g_call_timing_ex[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
struct AllocSnap {
    int64_t ns, calls;
    static AllocSnap now() { return AllocSnap{g_alloc_meter.ns.load(), g_alloc_meter.calls.load()}; }
    double seconds_since(const AllocSnap &a) const { return (double)(ns - a.ns) * 1e-9; }
};
// how the calling thread's last file-level call was carried out (bsig_last_call_route)
thread_local char g_call_route[320] = "";
inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------------------------------------
// What the file-level calls keep between calls (the reference re-opens file and index on every
// call, src/bamsignals.cpp:449,479; here the expensive part is the decode to HBM):
//   * the GPUs in use: one context (stream) per listed device;
//   * opened BAMs: header + parsed BAI of the last few files;
//   * resident BAMs: whole files decoded to HBM (on every listed GPU), least recently used first
//     out once their bytes exceed BAMSIGNALS_CACHE_GB per GPU (default 96).
// A file is identified by path + size + mtime (ns) of the BAM and of its index: a rewritten file is
// decoded again.  The lock is held for look-ups and updates only, never across a decode or a
// launch: calls from several host threads on resident BAMs run side by side (cold decodes take
// turns, they use the whole GPU anyway); an entry in use is kept alive by its shared_ptr.
// ---------------------------------------------------------------------------------------------
// Buffers the multi-GPU result path keeps between calls (so that a call on a resident BAM does no
// hipMalloc / hipFree / hipHostMalloc: config 5 moved 8 GB of allocations per call through the driver)
struct SlotScratch {
    int32_t *d_shard = nullptr;   size_t shard_cap = 0;      // this slot's result shard (device, int32 cells)
    int32_t *h_shard = nullptr;   size_t h_cap = 0;          // ... page-locked host copy ("pcie" gather)
};
struct RootScratch {
    int32_t *d_gather = nullptr;  size_t gather_cap = 0;     // RCCL receive buffer: the shards behind each other
    int32_t *d_final = nullptr;   size_t final_cap = 0;      // the result in the caller's range order
    int64_t *d_tab[3] = {nullptr, nullptr, nullptr};         // segment offsets, segment -> range, range offsets
    size_t tab_cap[3] = {0, 0, 0};
};
struct Slots {
    std::vector<int> devices;
    std::vector<bsig_ctx *> ctx;
    std::mutex run_mu;                   // one multi-GPU run at a time per device list (they share the scratch)
    std::vector<SlotScratch> scratch;
    RootScratch root;
    std::atomic<int64_t> scratch_allocs{0};   // device / pinned allocations made for the scratch (tests: stays flat)
    // the result-path buffers go back to the library's free blocks (the caller holds run_mu, or is the last owner)
    void release_scratch()
    {
        for (size_t k = 0; k < scratch.size(); ++k) {
            (void)hipSetDevice(devices[k]);
            if (scratch[k].d_shard) block_free(devices[k], scratch[k].d_shard, scratch[k].shard_cap * sizeof(int32_t));
            if (scratch[k].h_shard) (void)hipHostFree(scratch[k].h_shard);
            scratch[k] = SlotScratch{};
        }
        if (devices.empty()) return;
        (void)hipSetDevice(devices[0]);
        if (root.d_gather) block_free(devices[0], root.d_gather, root.gather_cap * sizeof(int32_t));
        if (root.d_final) block_free(devices[0], root.d_final, root.final_cap * sizeof(int32_t));
        for (int k = 0; k < 3; ++k)
            if (root.d_tab[k]) block_free(devices[0], root.d_tab[k], root.tab_cap[k] * sizeof(int64_t));
        root = RootScratch{};
    }
    ~Slots()
    {
        release_scratch();
        for (bsig_ctx *c : ctx) if (c) bsig_ctx_destroy(c);
    }
};
struct Resident {
    std::string key;                     // file key + '@' + device list
    std::shared_ptr<Slots> slots;        // the contexts the reads live on stay alive as long as the reads
    std::vector<bsig_reads *> reads;     // one per slot
    int64_t bytes = 0;                   // per GPU
    // index-driven decodes: the (rid, beg, end) intervals the reads were decoded for; a later query whose regions all
    // lie inside them can use these reads as they are
    Intervals cov;
    void free_reads() { for (bsig_reads *&r : reads) { if (r) bsig_reads_free(r); r = nullptr; } }
    ~Resident() { free_reads(); }
};
struct OpenBam {
    std::string key;
    bsig_bam *bam = nullptr;
    ~OpenBam() { if (bam) bsig_bam_close(bam); }
};

struct Cache {
    std::mutex mu;                                       // guards everything below
    std::mutex decode_mu;                                // cold decodes take turns
    std::vector<std::shared_ptr<Slots>> slot_sets;       // one per device list seen (an R session alternating
                                                         // between device= arguments keeps both sets resident)
    std::list<std::shared_ptr<OpenBam>> bams;            // most recently used first
    std::list<std::shared_ptr<Resident>> resident;       // whole files, most recently used first
    std::list<std::shared_ptr<Resident>> regional;       // index-driven decodes, most recently used first (few)
    // the first entry of that key (which `also` accepts), moved to the front; null if there is none.  Under mu.
    template <typename T, typename Also>
    static std::shared_ptr<T> touch(std::list<std::shared_ptr<T>> &l, const std::string &key, Also also)
    {
        for (auto it = l.begin(); it != l.end(); ++it)
            if ((*it)->key == key && also(**it)) {
                l.splice(l.begin(), l, it);
                return l.front();
            }
        return nullptr;
    }
    template <typename T>
    static std::shared_ptr<T> touch(std::list<std::shared_ptr<T>> &l, const std::string &key)
    {
        return touch(l, key, [](const T &) { return true; });
    }
    void clear()
    {
        resident.clear();
        regional.clear();
        bams.clear();
        slot_sets.clear();
    }
};
Cache g_cache;

// size + mtime (ns) of a file, "" if it cannot be examined
std::string file_stamp(const std::string &path)
{
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return std::string();
    return std::to_string((long long)st.st_size) + "|" + std::to_string((long long)st.st_mtime) + "|" +
           std::to_string((long long)st.st_mtim.tv_nsec);
}

std::string file_key(const std::string &path)
{
    const std::string s = file_stamp(path);
    return s.empty() ? s : path + "|" + s;
}

// size + mtime of every index file a BAM may be opened with (<bam>.csi, <stem>.csi, <bam>.bai, <stem>.bai;
// bsig_bam_open tries them in this order): whichever one is used, replacing, adding or removing it
// changes the stamp, so cached headers, resident reads and reads files are never tied to a stale index
std::string index_stamps(const std::string &bam)
{
    std::string stem = bam;
    if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".bam") == 0) stem.erase(stem.size() - 4);
    std::string out;
    for (const std::string &cand : {bam + ".bai", stem + ".bai", bam + ".csi", stem + ".csi"}) out += file_stamp(cand) + ";";
    return out;
}

int64_t cache_budget_bytes()
{
    double gb = 96.0;
    if (const char *e = getenv("BAMSIGNALS_CACHE_GB")) gb = std::max(0.0, atof(e));
    return (int64_t)(gb * (double)(1ull << 30));
}

// the reads file ("sidecar") of a BAM, or "" when sidecars are off: BAMSIGNALS_SIDECAR=1 puts it next
// to the BAM (<bam>.bsig), BAMSIGNALS_SIDECAR_DIR=<dir> into that directory
std::string sidecar_path(const std::string &bampath)
{
    if (const char *d = getenv("BAMSIGNALS_SIDECAR_DIR")) {
        if (!*d) return std::string();
        char real[4096];
        const std::string abs = realpath(bampath.c_str(), real) ? std::string(real) : bampath;
        uint64_t h = 1469598103934665603ull;                       // FNV-1a of the absolute path
        for (unsigned char ch : abs) { h ^= ch; h *= 1099511628211ull; }
        const size_t slash = abs.find_last_of('/');
        char hex[32];
        snprintf(hex, sizeof hex, "%016llx", (unsigned long long)h);
        return std::string(d) + "/" + abs.substr(slash == std::string::npos ? 0 : slash + 1) + "." + hex + ".bsig";
    }
    if (const char *e = getenv("BAMSIGNALS_SIDECAR"))
        if (*e && strcmp(e, "0") != 0) return bampath + ".bsig";
    return std::string();
}

// GPUs a file-level call uses: the `device` argument if >= 0, else BAMSIGNALS_DEVICES ("0,1,2,3":
// ranges are dealt round-robin to them), else BAMSIGNALS_DEVICE, else GPU 0
std::vector<int> pick_devices(int device)
{
    std::vector<int> d;
    if (device >= 0) return {device};
    if (const char *e = getenv("BAMSIGNALS_DEVICES")) {
        for (const char *p = e; *p;) {
            char *end = nullptr;
            const long v = strtol(p, &end, 10);
            if (end == p) break;
            d.push_back((int)v);
            p = *end == ',' ? end + 1 : end;
        }
    }
    if (d.empty()) d.push_back(getenv("BAMSIGNALS_DEVICE") ? atoi(getenv("BAMSIGNALS_DEVICE")) : 0);
    return d;
}

bool env_is(const char *name, const char *value)
{
    const char *e = getenv(name);
    return e && !strcmp(e, value);
}

// body(k) for every slot on its own host thread (one thread per GPU); the first failure wins and its
// message becomes the caller's bsig_last_error()
int for_each_slot(size_t n, const std::function<int(size_t)> &body)
{
    std::vector<int> rcs(n, BSIG_OK);
    std::vector<std::string> msgs(n);
    auto one = [&](size_t k) {
        rcs[k] = body(k);
        if (rcs[k]) msgs[k] = bsig_last_error();
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < n; ++k) {
        try { th.emplace_back(one, k); } catch (const std::system_error &) { one(k); }
    }
    one(0);
    for (auto &t : th) t.join();
    for (size_t k = 0; k < n; ++k)
        if (rcs[k]) return fail(rcs[k], "%s", msgs[k].c_str());
    return BSIG_OK;
}

// grows a cached buffer of the multi-GPU result path (never shrinks; released with the Slots).  The memory comes
// from the library's cache of free device blocks (runtime_internal.h): right after a cold decode that cache
// holds the decode's scratch, and a fresh hipMalloc at that moment is exactly the one that stalls for seconds
template <typename T>
int grow_dev(Slots &sl, int device, T **p, size_t *cap, size_t want)
{
    if (*p && *cap >= want) return BSIG_OK;
    HIP_TRY(hipSetDevice(device));
    if (*p) { block_free(device, *p, *cap * sizeof(T)); *p = nullptr; *cap = 0; }
    const size_t n = std::max<size_t>(want + want / 8, 1024);          // head-room: a slightly larger call fits too
    void *q = nullptr;
    size_t got = 0;
    HIP_TRY(block_alloc(device, n * sizeof(T), 2.0, &q, &got));
    *p = (T *)q;
    *cap = got / sizeof(T);
    sl.scratch_allocs.fetch_add(1);
    return BSIG_OK;
}
int grow_pinned(Slots &sl, int device, int32_t **p, size_t *cap, size_t want)
{
    if (*p && *cap >= want) return BSIG_OK;
    HIP_TRY(hipSetDevice(device));
    if (*p) { (void)hipHostFree(*p); *p = nullptr; *cap = 0; }
    const size_t n = std::max<size_t>(want + want / 8, 1024);
    HIP_TRY(hipHostMalloc((void **)p, n * sizeof(int32_t), hipHostMallocDefault));
    *cap = n;
    sl.scratch_allocs.fetch_add(1);
    return BSIG_OK;
}

// ranges as the four arrays a plan is made from
struct RangeView {
    int64_t n;
    const int32_t *rid, *loc, *width, *strand;
};
// ... a copy of those at the indices idx[a .. b)
struct RangeBlock {
    std::vector<int32_t> rid, loc, width, strand;
    RangeBlock() = default;
    RangeBlock(const std::vector<int64_t> &idx, int64_t a, int64_t b, const RangeView &g)
        : rid((size_t)(b - a)), loc((size_t)(b - a)), width((size_t)(b - a)), strand((size_t)(b - a))
    {
        for (int64_t i = a; i < b; ++i) {
            const int64_t j = idx[(size_t)i];
            rid[(size_t)(i - a)] = g.rid[j]; loc[(size_t)(i - a)] = g.loc[j]; width[(size_t)(i - a)] = g.width[j]; strand[(size_t)(i - a)] = g.strand[j];
        }
    }
    RangeView view() const { return RangeView{(int64_t)rid.size(), rid.data(), loc.data(), width.data(), strand.data()}; }
};

// a per-range plan of a file-level call: bsig_plan_create, or for reads resized to the fragment (frag_len != 0, judged by
// resized_rule before the BAM was opened) bsig_plan_create_resized
int plain_plan(bsig_ctx *ctx, const bsig_reads *reads, const RangeView &g, const FileCall &c, bsig_plan **plan)
{
    return c.frag_len ? bsig_plan_create_resized(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, &c.prm, c.frag_len, plan)
                      : bsig_plan_create(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, &c.prm, plan);
}
// a reduction's plan: the kind's bsig_plan_create_* call with the kind's own argument in its place
int reduction_plan(bsig_ctx *ctx, const bsig_reads *reads, const RangeView &g, const FileCall &c, bsig_plan **plan)
{
    const bsig_params *p = &c.prm;
    const int32_t arg = c.to.arg;
    switch (c.to.kind) {
    case Reduce::sum:
        return c.frag_len ? bsig_plan_create_sum_resized(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, c.frag_len, plan)
                          : bsig_plan_create_sum(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, plan);
    case Reduce::xcorr: return bsig_plan_create_xcorr(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, arg, plan);
    case Reduce::frag: return bsig_plan_create_frag(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, arg, plan);
    case Reduce::hist: return bsig_plan_create_hist(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, arg, plan);
    case Reduce::summary: return bsig_plan_create_summary(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, arg, c.to.thresholds, plan);
    case Reduce::scaled: return bsig_plan_create_scaled(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, arg, plan);
    case Reduce::vplot: return bsig_plan_create_vplot(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, arg, plan);
    case Reduce::capped: return bsig_plan_create_capped(ctx, reads, g.n, g.rid, g.loc, g.width, g.strand, p, arg, c.frag_len, plan);
    case Reduce::none: break;
    }
    return fail(BSIG_ERR_ARG, "not a reduction");
}

// What the stages of one file-level call hand on to each other; lives on file_level's stack.
struct Stage {
    const FileCall &call;
    double *T, *X;                          // the calling thread's timing slots
    int64_t cells = 0, row = 0;             // judge_call: a reduction's cells, and those of one range (summaries, scaled regions)
    std::string key, bkey;                  // open_cached_bam: the BAM's stamp, with its index files'; "" if it cannot be examined
    std::shared_ptr<OpenBam> ob;
    std::vector<int32_t> rid, loc;          // resolve_ranges: reference ids and 0-based starts, the plan's rule, the destination
    PlanRule rule;
    HostDest dest;
    std::vector<int64_t> own_off;
    std::shared_ptr<Slots> slots;           // slots_for: the GPUs, whether the multi-GPU routes are taken, the reads' cache key
    bool many = false;
    std::string rkey;
    std::vector<int32_t> ref_map;           // resolve_gene_references: for every reference of the BAM the model's, or -1
    std::shared_ptr<Resident> res;          // acquire_reads: the reads on every slot and where they came from
    std::string how_decoded = "resident";
    RangeView ranges() const { return RangeView{call.at.n, rid.data(), loc.data(), call.at.width, call.at.strand}; }
};

// ---- several GPUs: ranges are independent (each owns its output, ref: src/bamsignals.cpp:164,181,186)
// The (rid, loc)-sorted ranges (ref: :222-226,246) are dealt in blocks to the GPUs (rangemath.h: deal_shards); every GPU
// plans and runs its shard on its own stream, driven by its own host thread, into a shard buffer the slot keeps between
// calls.  The shards then reach the caller by one of
//   "pcie/blocks" (env BAMSIGNALS_GATHER=blocks, or by itself where the shards' contiguous slices of the caller's result are
//                 long): every slice over its own GPU's PCIe link straight to its place;
//   "xgmi/rccl"   (default where RCCL runs): RCCL grouped send/recv into a receive buffer on the first GPU
//                 (collect.h), put into the caller's range order there by k_place_segments, ONE download;
//   "xgmi/direct" (default without RCCL where the first GPU can read its peers; env BAMSIGNALS_GATHER=direct):
//                 k_place_segments on the first GPU reads every peer's shard buffer in place over xGMI --
//                 one pass, no receive buffer -- then ONE download;
//   "xgmi/peer":  as rccl with hipMemcpyPeerAsync (no RCCL, no peer mapping);
//   "pcie"        (env BAMSIGNALS_GATHER=pcie): every shard over its own GPU's PCIe link into a page-locked
//                 buffer, put in place by host threads (bsig_scatter_segments).
// All device and page-locked buffers are kept in the Slots: a call on a resident BAM allocates nothing here.
struct ShardRun {
    Slots &sl;
    const Stage &s;
    ShardDeal deal;
    std::vector<RangeBlock> ranges;         // per slot, in the shard's order
    std::vector<bsig_plan *> plan;          // ... its plan, freed when the run goes out of scope
    std::vector<int64_t> cells;
    ShardRun(Slots &sl_, const Stage &s_) : sl(sl_), s(s_) {}
    ~ShardRun() { for (bsig_plan *p : plan) if (p) bsig_plan_free(p); }
    size_t nd() const { return sl.ctx.size(); }
};

// slot k plans its shard, checks it against the caller's offsets and launches it into the slot's shard buffer
int plan_and_run_slot(ShardRun &R, size_t k)
{
    Slots &sl = R.sl;
    const std::vector<int64_t> &which = R.deal.which[k];
    int r = plain_plan(sl.ctx[k], R.s.res->reads[k], R.ranges[k].view(), R.s.call, &R.plan[k]);
    if (r) return r;
    R.cells[k] = bsig_plan_cells(R.plan[k]);
    // every segment must fit its destination: the caller's offsets are only trusted after this check
    const int64_t *po = bsig_plan_offsets(R.plan[k]), *off = R.s.dest.off;
    for (size_t j = 0; j < which.size(); ++j)
        if (po[j + 1] - po[j] != off[which[j] + 1] - off[which[j]])
            return fail(BSIG_ERR_ARG, "offsets do not match bsig_layout() for these parameters");
    SlotScratch &X = sl.scratch[k];
    r = grow_dev(sl, sl.devices[k], &X.d_shard, &X.shard_cap, (size_t)std::max<int64_t>(R.cells[k], 4));
    if (r) return r;
    r = bsig_plan_run(R.plan[k], X.d_shard);
    if (r) return r;
    return plan_check_overflow(R.plan[k]);       // (binned coverage with heavy slices only: waits for the run)
}

// "pcie/blocks", on slot k's thread: every contiguous slice of the caller's result this GPU owns leaves over this GPU's own
// PCIe link, straight to its place: no gather on one GPU, no reassembly pass on the host
int deliver_blocks(ShardRun &R, size_t k, int copy_thr, double *t_run_done)
{
    const int r = bsig_ctx_sync(R.sl.ctx[k]);
    if (r) return r;
    *t_run_done = now_s();
    const int64_t *po = bsig_plan_offsets(R.plan[k]), *off = R.s.dest.off;
    std::vector<int64_t> s0, d0, nc;
    for (const SegRun &q : R.deal.runs[k]) {
        s0.push_back(po[q.j0]); d0.push_back(off[R.deal.which[k][(size_t)q.j0]]); nc.push_back(po[q.j1] - po[q.j0]);
    }
    return download_slices_to_dest(R.sl.ctx[k], R.sl.scratch[k].d_shard, (int64_t)s0.size(), s0.data(), d0.data(), nc.data(), R.s.dest, copy_thr);
}

// "pcie": slot k's shard into its page-locked buffer (on the slot's thread), then all of them put in place by host threads
int pcie_download_slot(ShardRun &R, size_t k)
{
    SlotScratch &X = R.sl.scratch[k];
    if (R.cells[k]) {
        const int r = grow_pinned(R.sl, R.sl.devices[k], &X.h_shard, &X.h_cap, (size_t)R.cells[k]);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(X.h_shard, X.d_shard, (size_t)R.cells[k] * sizeof(int32_t), hipMemcpyDeviceToHost,
                               (hipStream_t)bsig_ctx_stream(R.sl.ctx[k])));
    }
    return bsig_ctx_sync(R.sl.ctx[k]);
}
int deliver_pcie(ShardRun &R)
{
    int rc = BSIG_OK;
    for (size_t k = 0; k < R.nd() && rc == BSIG_OK; ++k)
        rc = scatter_segments_to((int64_t)R.deal.which[k].size(), R.sl.scratch[k].h_shard, bsig_plan_offsets(R.plan[k]), R.s.dest,
                                 R.deal.which[k].data());
    return rc;
}

// "xgmi": the shards meet on the first GPU, in the caller's range order, and leave in one download.  *t_placed, *t_down:
// when the result stood on the first GPU, and when it had reached the host
int deliver_xgmi(ShardRun &R, int64_t total, std::string &gather_name, double *t_placed, double *t_down)
{
    Slots &sl = R.sl;
    const size_t nd = R.nd();
    const int64_t n = R.s.call.at.n;
    RootScratch &G = sl.root;
    const int dev0 = sl.devices[0];
    hipStream_t st = (hipStream_t)bsig_ctx_stream(sl.ctx[0]);
    // tables: per shard its local segment offsets (n_k + 1 entries) and segment -> range; the ranges' offsets
    std::vector<int64_t> seg_off, seg_which;
    seg_off.reserve((size_t)n + nd);
    seg_which.reserve((size_t)n);
    std::vector<size_t> seg_base(nd), which_base(nd);
    for (size_t k = 0; k < nd; ++k) {
        seg_base[k] = seg_off.size();
        which_base[k] = seg_which.size();
        const int64_t *po = bsig_plan_offsets(R.plan[k]);
        seg_off.insert(seg_off.end(), po, po + R.deal.which[k].size() + 1);
        seg_which.insert(seg_which.end(), R.deal.which[k].begin(), R.deal.which[k].end());
    }
    int r = grow_dev(sl, dev0, &G.d_final, &G.final_cap, (size_t)total);
    if (!r) r = grow_dev(sl, dev0, &G.d_tab[0], &G.tab_cap[0], seg_off.size());
    if (!r) r = grow_dev(sl, dev0, &G.d_tab[1], &G.tab_cap[1], std::max<size_t>(seg_which.size(), 1));
    if (!r) r = grow_dev(sl, dev0, &G.d_tab[2], &G.tab_cap[2], (size_t)n + 1);
    if (r) return r;
    HIP_TRY(hipSetDevice(dev0));
    HIP_TRY(hipMemcpyAsync(G.d_tab[0], seg_off.data(), seg_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(G.d_tab[1], seg_which.data(), seg_which.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(G.d_tab[2], R.s.dest.off, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    ExchangeUse use;            // holds the exchange's lock until the streams are synchronised below
    r = exchange_open(sl.ctx, use);
    if (r) return r;
    // (env BAMSIGNALS_GATHER=direct: in-place reads even where RCCL runs; =copy: a receive buffer even where
    // in-place reads are possible -- both exist so that an 8-GPU node can time all three)
    const bool want_direct = env_is("BAMSIGNALS_GATHER", "direct"), want_copy = env_is("BAMSIGNALS_GATHER", "copy");
    const bool rccl = !strcmp(use.transport, "rccl") && !want_direct;
    const bool direct = !rccl && !want_copy && exchange_root_reads_peers(use);
    std::vector<const int32_t *> from(nd);          // where the place kernel finds shard k
    if (direct) {
        for (size_t k = 0; k < nd; ++k) from[k] = sl.scratch[k].d_shard;
        gather_name = "xgmi/direct";
    } else {
        r = grow_dev(sl, dev0, &G.d_gather, &G.gather_cap, (size_t)total);
        if (r) return r;
        std::vector<size_t> goff(nd), glen(nd);
        std::vector<const uint8_t *> src(nd);
        int64_t at = 0;
        for (size_t k = 0; k < nd; ++k) {
            goff[k] = (size_t)at * sizeof(int32_t);
            glen[k] = (size_t)R.cells[k] * sizeof(int32_t);
            src[k] = (const uint8_t *)sl.scratch[k].d_shard;
            from[k] = G.d_gather + at;
            at += R.cells[k];
        }
        // (the first GPU's own shard is read in place: no copy into the receive buffer)
        from[0] = sl.scratch[0].d_shard;
        glen[0] = 0;
        r = exchange_gather(use, src, glen, (uint8_t *)G.d_gather, goff);
        if (r) return r;
        gather_name = std::string("xgmi/") + use.transport;
        for (size_t k = 1; k < nd; ++k) {              // the senders' streams (RCCL queues the sends there)
            r = bsig_ctx_sync(sl.ctx[k]);
            if (r) return r;
        }
    }
    HIP_TRY(hipSetDevice(dev0));
    for (size_t k = 0; k < nd; ++k)
        HIP_TRY(launch_place_segments((int64_t)R.deal.which[k].size(), from[k], G.d_tab[0] + seg_base[k], G.d_final, G.d_tab[2],
                                      G.d_tab[1] + which_base[k], st));
    HIP_TRY(hipStreamSynchronize(st));
    use.release();
    *t_placed = now_s();
    r = download_to_dest(sl.ctx[0], G.d_final, R.s.dest, total);
    *t_down = now_s();
    return r;
}

// The per-range result of a call over several slots: deal, plan and run on every slot, deliver by the route of the day.
int run_on_slots(const Stage &s, std::string &gather_name)
{
    Slots &sl = *s.slots;
    const int64_t n = s.call.at.n, *off = s.dest.off;
    std::lock_guard<std::mutex> run_lock(sl.run_mu);
    const double t0 = now_s();
    const size_t nd = sl.ctx.size();
    if (sl.scratch.size() != nd) sl.scratch.resize(nd);
    std::vector<int64_t> order;
    sort_ranges(n, s.rid.data(), s.loc.data(), order);
    int64_t block = default_shard_block(n, nd);
    if (const char *e = getenv("BAMSIGNALS_SHARD_BLOCK")) block = std::max<int64_t>(1, atoll(e));      // (1 = round-robin, range by range)
    ShardRun R(sl, s);
    R.deal = deal_shards(n, order, nd, block);
    R.plan.assign(nd, nullptr);
    R.cells.assign(nd, 0);
    for (size_t k = 0; k < nd; ++k) R.ranges.emplace_back(R.deal.which[k], 0, (int64_t)R.deal.which[k].size(), s.ranges());
    // "blocks": by request, or by itself where the slices are long (64 ranges or more on average) and the result
    // is large enough for the route to matter
    const char *genv = getenv("BAMSIGNALS_GATHER");
    if (genv && !*genv) genv = nullptr;
    const bool blocks = genv ? !strcmp(genv, "blocks") : (R.deal.n_runs * 64 <= n && off[n] * (int64_t)sizeof(int32_t) >= ((int64_t)32 << 20));
    const bool pcie = env_is("BAMSIGNALS_GATHER", "pcie");
    gather_name = blocks ? "pcie/blocks" : pcie ? "pcie" : "xgmi";
    // host threads that move page-locked halves on, per GPU: all GPUs download at once (slots that name the same
    // GPU take turns on its staging halves, each with the device's full share of threads)
    std::vector<int> distinct(sl.devices);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    int copy_total = 16;
    if (const char *e = getenv("BAMSIGNALS_COPY_THREADS")) copy_total = std::max(1, std::min(64, atoi(e)));
    const int copy_thr = std::max(2, copy_total / (int)std::max<size_t>(distinct.size(), 1));
    std::vector<double> t_run_done(nd, 0.0);
    // one host thread per GPU
    int rc = for_each_slot(nd, [&](size_t k) -> int {
        const int r = plan_and_run_slot(R, k);
        if (r) return r;
        if (blocks) return deliver_blocks(R, k, copy_thr, &t_run_done[k]);
        return pcie ? pcie_download_slot(R, k) : bsig_ctx_sync(sl.ctx[k]);
    });
    if (rc) return rc;
    const double t1 = now_s();
    int64_t cells = 0;
    for (size_t k = 0; k < nd; ++k) cells += R.cells[k];
    const int64_t total = off[n];
    if (cells != total) return fail(BSIG_ERR_ARG, "offsets do not match bsig_layout() for these parameters");
    char times[128] = "";
    if (blocks) {
        double t_run = t0;
        for (double t : t_run_done) t_run = std::max(t_run, t);
        snprintf(times, sizeof times, " (plan+run %.3f s, download in %lld slices %.3f s)", t_run - t0, (long long)R.deal.n_runs, t1 - t_run);
    } else if (pcie) {
        rc = deliver_pcie(R);
        snprintf(times, sizeof times, " (plan+run+d2h %.3f s, host scatter %.3f s)", t1 - t0, now_s() - t1);
    } else if (total) {
        double t2 = t1, t3 = t1;
        rc = deliver_xgmi(R, total, gather_name, &t2, &t3);
        if (rc) for (size_t k = 0; k < nd; ++k) (void)bsig_ctx_sync(sl.ctx[k]);
        snprintf(times, sizeof times, " (plan+run %.3f s, gather+place %.3f s, download %.3f s)", t1 - t0, t2 - t1, t3 - t2);
    }
    gather_name += times;
    return rc;
}

// Out of device memory: what the cache can spare goes back to the driver -- the index-driven decodes it keeps, the
// result-path buffers of device lists nobody is running on (never those of `keep`, the caller's own), and the free
// blocks.  What a running call holds stays (shared_ptr, run_mu).
void drop_spare_device_memory(const Slots *keep)
{
    std::list<std::shared_ptr<Resident>> drop;
    std::vector<std::shared_ptr<Slots>> sets;
    {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        drop.swap(g_cache.regional);
        sets = g_cache.slot_sets;
    }
    drop.clear();
    for (auto &sp : sets) {
        if (sp.get() == keep) continue;
        std::unique_lock<std::mutex> run(sp->run_mu, std::try_to_lock);
        if (run.owns_lock()) sp->release_scratch();
    }
    block_cache_release();
}

// A reduction over the ranges, its result s.cells int64.  row == 0: every cell is a sum over ranges -- the sum
// (bsig_pileup_sum / bsig_coverage_sum), the strand cross-correlation (bsig_pileup_xcorr), the fragment-length histogram
// (bsig_pileup_frag), the depth histogram (bsig_pileup_hist / bsig_coverage_hist), the V-plot (bsig_pileup_vplot).  row > 0: every range is reduced by itself
// to a row of `row` int64 (S * (3 + K), S * n_bins) -- the per-range summaries and the scaled regions (bsig_*_summary,
// bsig_*_scaled).  One GPU takes all ranges (route `what`); several take a block of the sorted ranges each, and the host ADDS
// the blocks' int64 vectors or PLACES a block's rows at the caller's indices -- no per-base cell leaves a GPU.
// The capped signals (bsig_pileup_capped / bsig_coverage_capped) take the same route with int32 cells: their rows are of
// unequal length, so a block's rows are placed through the layout's offsets (capped_on_slots).
int capped_on_slots(const Stage &s, std::string &route)
{
    const FileCall &c = s.call;
    const std::vector<bsig_reads *> &reads = s.res->reads;
    const RangeView g = s.ranges();
    int32_t *out = c.to.out;
    const int64_t *off = c.to.off;
    const size_t nd = reads.size();
    if (nd == 1) {
        const double t0 = now_s();
        bsig_plan *plan = nullptr;
        int rc = reduction_plan(s.slots->ctx[0], reads[0], g, c, &plan);
        s.X[3] = now_s() - t0;
        if (rc == BSIG_OK) rc = plan_run_reduced_to_host(plan, out, &s.X[4], &s.X[5]);
        if (plan) bsig_plan_free(plan);
        route = "capped";
        return rc;
    }
    std::vector<int64_t> order;
    sort_ranges(g.n, g.rid, g.loc, order);
    const int rc = for_each_slot(nd, [&](size_t k) -> int {
        int64_t a, b;
        slot_block(g.n, k, nd, &a, &b);
        if (a >= b) return BSIG_OK;
        const RangeBlock B(order, a, b, g);
        bsig_plan *plan = nullptr;
        int rk = reduction_plan(s.slots->ctx[k], reads[k], B.view(), c, &plan);
        std::vector<int32_t> part;
        if (rk == BSIG_OK) {
            try {
                part.resize((size_t)bsig_plan_cells(plan));
            } catch (const std::bad_alloc &) {
                rk = fail(BSIG_ERR_NOMEM, "out of host memory for %lld result cells", (long long)bsig_plan_cells(plan));
            }
        }
        if (rk == BSIG_OK) rk = plan_run_reduced_to_host(plan, part.data());
        if (rk == BSIG_OK) {    // (the blocks' ranges are disjoint: every slot writes rows of its own)
            const int64_t *po = bsig_plan_offsets(plan);
            for (int64_t i = a; i < b && rk == BSIG_OK; ++i) {
                const int64_t j = order[(size_t)i], len = po[i - a + 1] - po[i - a];
                if (len != off[j + 1] - off[j]) rk = fail(BSIG_ERR_ARG, "offsets do not match bsig_layout() for these parameters");
                else std::copy(part.begin() + po[i - a], part.begin() + po[i - a + 1], out + off[j]);
            }
        }
        if (plan) bsig_plan_free(plan);
        return rk;
    });
    if (rc != BSIG_OK) return rc;
    route = "capped of " + std::to_string(nd) + " blocks of ranges, rows placed on the host";
    return BSIG_OK;
}
int reduced_on_slots(const Stage &s, std::string &route)
{
    const FileCall &c = s.call;
    if (c.to.kind == Reduce::capped) return capped_on_slots(s, route);
    const std::vector<bsig_reads *> &reads = s.res->reads;
    const RangeView g = s.ranges();
    const int64_t cells = s.cells, row = s.row;
    int64_t *out = c.to.reduced;
    const char *what = c.to.kind == Reduce::scaled ? "scaled" : c.to.kind == Reduce::summary ? "summary" : "sum";
    const size_t nd = reads.size();
    if (nd == 1) {
        const double t0 = now_s();
        bsig_plan *plan = nullptr;
        int rc = reduction_plan(s.slots->ctx[0], reads[0], g, c, &plan);
        s.X[3] = now_s() - t0;
        if (rc == BSIG_OK) rc = plan_run_reduced_to_host(plan, out, &s.X[4], &s.X[5]);
        if (plan) bsig_plan_free(plan);
        route = what;
        return rc;
    }
    std::vector<int64_t> order;
    sort_ranges(g.n, g.rid, g.loc, order);
    if (!row) std::fill(out, out + cells, (int64_t)0);     // (a call tried again after BSIG_ERR_NOMEM adds from zero)
    std::mutex adding;
    const int rc = for_each_slot(nd, [&](size_t k) -> int {
        int64_t a, b;
        slot_block(g.n, k, nd, &a, &b);
        if (a >= b) return BSIG_OK;
        const RangeBlock B(order, a, b, g);
        const int64_t part_cells = row ? (b - a) * row : cells;
        std::vector<int64_t> part;
        try {
            part.resize((size_t)part_cells);
        } catch (const std::bad_alloc &) {
            return fail(BSIG_ERR_NOMEM, "out of host memory for %lld result cells", (long long)part_cells);
        }
        bsig_plan *plan = nullptr;
        int rk = reduction_plan(s.slots->ctx[k], reads[k], B.view(), c, &plan);
        if (rk == BSIG_OK) rk = plan_run_reduced_to_host(plan, part.data());
        if (plan) bsig_plan_free(plan);
        if (rk != BSIG_OK) return rk;
        if (row) {      // (the blocks' ranges are disjoint: every slot writes rows of its own)
            for (int64_t i = a; i < b; ++i)
                std::copy(part.begin() + (i - a) * row, part.begin() + (i - a + 1) * row, out + order[(size_t)i] * row);
        } else {
            std::lock_guard<std::mutex> lock(adding);
            for (int64_t q = 0; q < cells; ++q) out[q] += part[(size_t)q];
        }
        return BSIG_OK;
    });
    if (rc != BSIG_OK) return rc;
    route = std::string(what) + " of " + std::to_string(nd) + " blocks of ranges, " + (row ? "rows placed on the host" : "added on the host");
    return BSIG_OK;
}

// a block's result in `buf` encoded on its device (*t_encoded: when that was done); the seg_off and the value columns of
// the block to the host
int encode_block(const Encoder &enc, bsig_plan *plan, const int32_t *buf, EncodedColumns &B, double *t_encoded)
{
    int64_t n = 0;
    int rc;
    auto size_cols = [&] {
        for (int c = 0; c < enc.n_cols; ++c) B.col[c].resize((size_t)n * enc.elem[c]);
    };
    if (enc.kind == EncoderKind::views) {
        bsig_views *v = nullptr;
        rc = bsig_plan_views_create(plan, &v);
        if (rc == BSIG_OK) rc = bsig_views_encode(v, buf, enc.lower, enc.upper, &n);
        *t_encoded = now_s();
        if (rc == BSIG_OK) {
            size_cols();
            rc = bsig_views_fetch(v, B.seg_off.data(), (int32_t *)B.col[0].data(), (int32_t *)B.col[1].data(), (int64_t *)B.col[2].data(),
                                  (int32_t *)B.col[3].data(), (int32_t *)B.col[4].data());
        }
        if (v) bsig_views_free(v);
    } else {
        bsig_runs *r = nullptr;
        rc = bsig_plan_runs_create(plan, &r);
        if (rc == BSIG_OK) rc = bsig_runs_encode(r, buf, &n);
        *t_encoded = now_s();
        if (rc == BSIG_OK) {
            size_cols();
            rc = bsig_runs_fetch(r, B.seg_off.data(), (int32_t *)B.col[0].data(), (int32_t *)B.col[1].data());
        }
        if (r) bsig_runs_free(r);
    }
    return rc;
}

// cells per block of ranges whose per-base result is in HBM at one time (bsig_pileup_runs / bsig_coverage_runs)
int64_t runs_block_cells()
{
    if (const char *e = getenv("BAMSIGNALS_RUNS_BLOCK_CELLS")) {      // (read per call: tests force many blocks)
        const long long v = atoll(e);
        if (v >= 1) return (int64_t)v;
    }
    return (int64_t)1 << 31;
}

// a block of the sorted ranges on its way through an encoder: where it was cut, and what came back
struct EncodedBlock : EncodedColumns {
    CellBlock at;
};

// slot k's blocks, one after the other through one device buffer: plan, run, overflow check, encode, fetch
int encode_slot_blocks(const Stage &s, size_t k, const std::vector<int64_t> &order, std::vector<EncodedBlock> &blocks)
{
    bsig_ctx *ctx = s.slots->ctx[k];
    const size_t nd = s.res->reads.size();
    const size_t S = s.rule.ss ? 2 : 1;
    int64_t max_cells = 0;
    for (const EncodedBlock &B : blocks)
        if (B.at.slot == k) max_cells = std::max(max_cells, B.at.cells);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(BSIG_ERR_DEVICE, "cannot select GPU %d", ctx->device);
    void *buf = nullptr;
    size_t got = 0;
    if (max_cells > 0) {
        const hipError_t e = block_alloc(ctx->device, (size_t)max_cells * sizeof(int32_t), 1.125, &buf, &got);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? BSIG_ERR_NOMEM : BSIG_ERR_DEVICE, "no device memory for a block of %lld cells: %s",
                        (long long)max_cells, hipGetErrorString(e));
    }
    int rk = BSIG_OK;
    for (EncodedBlock &B : blocks) {
        if (B.at.slot != k || rk != BSIG_OK) continue;
        const RangeBlock G(order, B.at.a, B.at.b, s.ranges());
        const double t0 = now_s();
        bsig_plan *plan = nullptr;
        rk = plain_plan(ctx, s.res->reads[k], G.view(), s.call, &plan);
        if (rk == BSIG_OK && bsig_plan_cells(plan) != B.at.cells) rk = fail(BSIG_ERR_ARG, "a block's cells do not match its plan's");
        const double t1 = now_s();
        if (rk == BSIG_OK) rk = bsig_plan_run(plan, (int32_t *)buf);
        if (rk == BSIG_OK) rk = bsig_ctx_sync(ctx);
        // (a bin past INT32_MAX fails the call before anything is encoded)
        if (rk == BSIG_OK) rk = plan_check_overflow(plan);
        double t2 = now_s();
        if (rk == BSIG_OK) {
            B.seg_off.resize((size_t)(B.at.b - B.at.a) * S + 1);
            rk = encode_block(s.call.to.enc, plan, (const int32_t *)buf, B, &t2);
        }
        if (nd == 1) { s.X[3] += t1 - t0; s.X[4] += t2 - t1; s.X[5] += now_s() - t2; }
        if (plan) bsig_plan_free(plan);
    }
    if (buf) block_free(ctx->device, buf, got);
    return rk;
}

// the blocks' segments in the caller's order: count, scan, copy
void order_segments(const std::vector<EncodedBlock> &blocks, const std::vector<int64_t> &order, int64_t n, int64_t S, const Encoder &enc,
                    EncodedColumns &out)
{
    out.n_seg = n * S;
    out.seg_off.assign((size_t)(n * S) + 1, 0);
    for (const EncodedBlock &B : blocks)
        for (int64_t t = 0; t < B.at.b - B.at.a; ++t)
            for (int64_t a = 0; a < S; ++a)
                out.seg_off[(size_t)(order[(size_t)(B.at.a + t)] * S + a) + 1] = B.seg_off[(size_t)(t * S + a) + 1] - B.seg_off[(size_t)(t * S + a)];
    for (int64_t k = 0; k < n * S; ++k) out.seg_off[(size_t)k + 1] += out.seg_off[(size_t)k];
    for (int c = 0; c < enc.n_cols; ++c) out.col[c].resize((size_t)out.seg_off.back() * enc.elem[c]);
    for (const EncodedBlock &B : blocks)
        for (int64_t t = 0; t < B.at.b - B.at.a; ++t) {
            // (a range's segments are neighbours on both sides)
            const int64_t from = B.seg_off[(size_t)(t * S)], cnt = B.seg_off[(size_t)((t + 1) * S)] - from;
            const int64_t to = out.seg_off[(size_t)(order[(size_t)(B.at.a + t)] * S)];
            for (int c = 0; cnt && c < enc.n_cols; ++c)
                memcpy(out.col[c].data() + (size_t)to * enc.elem[c], B.col[c].data() + (size_t)from * enc.elem[c], (size_t)cnt * enc.elem[c]);
        }
}

// The per-range result as runs or views (bsig_pileup_runs / bsig_coverage_runs, bsig_pileup_views / bsig_coverage_views).
// Each GPU takes a contiguous share of the (rid, loc)-sorted ranges, cut into blocks of at most runs_block_cells() cells
// (rangemath.h: cut_blocks): a block's plan runs into a device buffer, the overflow flag is checked, the buffer is encoded
// (runs.hip / views.hip) and only the encoder's result is downloaded.  The host puts the segments in the caller's order.
int encoded_on_slots(const Stage &s, std::string &route)
{
    const RangeView g = s.ranges();
    const size_t nd = s.res->reads.size();
    const int64_t S = s.rule.ss ? 2 : 1;
    std::vector<int64_t> order;
    sort_ranges(g.n, g.rid, g.loc, order);
    std::vector<int64_t> cells((size_t)g.n);
    for (int64_t i = 0; i < g.n; ++i) {
        const int32_t w = g.width[order[(size_t)i]];
        cells[(size_t)i] = w > 0 ? S * (((int64_t)w + s.rule.binsize - 1) / s.rule.binsize) : 0;
    }
    std::vector<EncodedBlock> blocks;
    for (const CellBlock &cut : cut_blocks(cells, nd, runs_block_cells())) {
        blocks.emplace_back();
        blocks.back().at = cut;
    }
    for (int k = 3; k < 6; ++k) s.X[k] = 0;
    const int rc = for_each_slot(nd, [&](size_t k) -> int { return encode_slot_blocks(s, k, order, blocks); });
    if (rc != BSIG_OK) return rc;
    order_segments(blocks, order, g.n, S, s.call.to.enc, *s.call.to.runs);
    route = std::string(s.call.to.enc.noun) + " of " + std::to_string(blocks.size()) + " block(s) of ranges, put in order on the host";
    return BSIG_OK;
}

// ---- the stages of a file-level call --------------------------------------------------------------------------------

// Stage 1, before any I/O: the entry point's own conditions, the arguments every call needs, then the kind's conditions --
// for the kinds that say so the plan's rule as well -- and the reduction's cells, zeroed.
int judge_call(const FileCall &c, Stage &s)
{
    const FileDest &to = c.to;
    const RangeArgs &at = c.at;
    using Shape = FileDest::Shape;
    // (what an entry point refuses of its own leaves the route of the thread's call before standing, as it always has)
    if (to.shape == Shape::into && !to.dst) return fail(BSIG_ERR_ARG, "destinations missing");
    if (to.shape == Shape::reduced && to.kind != Reduce::capped && !to.reduced) return fail(BSIG_ERR_ARG, "%s is NULL", to.name);
    CappedShape capped{};
    if (to.kind == Reduce::capped) {
        // the capped signals' own refusals come first of all: keep_dup, single ends, the fragment length and its mode
        if (const int rk = capped_shape(c.prm, to.arg, c.frag_len, &capped)) return rk;
        if (!to.out) return fail(BSIG_ERR_ARG, "out is NULL");
    }
    if (to.shape == Shape::encoded && to.enc.kind == EncoderKind::views && to.enc.lower > to.enc.upper)
        return fail(BSIG_ERR_ARG, "lower (%d) is above upper (%d)", (int)to.enc.lower, (int)to.enc.upper);
    if (c.overlap && c.overlap_type != 0 && c.overlap_type != 1) return fail(BSIG_ERR_ARG, "overlap type must be 0 (any) or 1 (within)");
    if (c.filter_missing) return fail(BSIG_ERR_ARG, "tlen_filter missing");
    if (to.shape == Shape::junctions) {
        if (!to.junctions) return fail(BSIG_ERR_ARG, "result is NULL");
        if (const int rk = junctions_rule(to.arg)) return rk;
    }
    if (to.shape == Shape::nucleotides)
        if (const int rk = nucleotides_rule(to.arg)) return rk;
    if (to.shape == Shape::sites) {
        if (!to.sites) return fail(BSIG_ERR_ARG, "result is NULL");
        if (const int rk = sites_rule(to.arg, to.site_rule[0], to.site_rule[1], to.site_rule[2], to.site_rule[3], to.site_rule[4])) return rk;
        if (const int rk = sites_ref_rule(at.n > 0 && at.width ? at.n : 0, at.width, to.site_ref)) return rk;
    }
    if (to.shape == Shape::genes) {
        if (const int rk = gene_counts_rule(to.model, to.arg, to.gene_counts, to.gene_summary)) return rk;
        if (at.n_levels != to.model->host.n_ref)
            return fail(BSIG_ERR_ARG, "the gene model has %d references, %d sequence names were given", (int)to.model->host.n_ref, (int)at.n_levels);
        if (at.n_levels > 0 && !at.levels) return fail(BSIG_ERR_ARG, "sequence names missing");
    }
    if (c.spliced) {
        // what bsig_plan_create would refuse on spliced reads, before any I/O: only the coverage of the blocks as they lie
        if (c.prm.mode != BSIG_MODE_COVERAGE && c.prm.mode != BSIG_MODE_COVERAGE_EX)
            return fail(BSIG_ERR_ARG, "spliced reads give coverage only: a block's start is not a read's 5' end");
        if (c.prm.tspan) return fail(BSIG_ERR_ARG, "spliced reads: tspan would extend every block of a read to the whole fragment");
        if (c.resized || c.frag_len) return fail(BSIG_ERR_ARG, "spliced reads: frag_len would resize every block of a read, not the read");
        if (to.kind != Reduce::none && to.kind != Reduce::sum)
            return fail(BSIG_ERR_ARG, "spliced reads: only the per-range coverage, its sum, its runs and its views are built");
    }
    PlanRule early;
    int rc = c.resized ? resized_rule(c.prm, c.frag_len) : (int)BSIG_OK;
    if (rc == BSIG_OK && c.rule_first) rc = check_params(c.prm, at.n > 0 && at.width ? at.n : 0, at.width, &early, c.frag_len);
    if (rc) return rc;
    g_call_route[0] = 0;        // (a refused call has no route)
    if (!at.bampath) return fail(BSIG_ERR_ARG, "bampath is NULL");
    if (at.n < 0 || (at.n > 0 && (!at.seq_code || !at.start || !at.width || !at.strand || !at.levels)))
        return fail(BSIG_ERR_ARG, "range arrays missing");
    if (to.shape == Shape::flat && !to.off) return fail(BSIG_ERR_ARG, "offsets missing");
    SumShape sum{};
    XcorrShape xcorr{};
    FragShape frag{};
    HistShape hist{};
    SummaryShape summary{};
    ScaledShape scaled{};
    VplotShape vplot{};
    switch (to.kind) {
    case Reduce::none:
        if (!to.runs) break;
        if (c.prm.mode == BSIG_MODE_COUNT) return fail(BSIG_ERR_ARG, "bamCount has no %s: one cell per range", to.enc.noun);
        rc = check_params(c.prm, at.n, at.width, &early, c.frag_len);
        break;
    case Reduce::sum:
        rc = sum_shape(c.prm, at.n, at.width, &sum);
        s.cells = sum.cells;
        break;
    case Reduce::xcorr:
        rc = xcorr_shape(c.prm, to.arg, &xcorr);
        s.cells = xcorr.cells;
        break;
    case Reduce::frag:
        rc = frag_shape(c.prm, to.arg, &frag);
        s.cells = frag.cells;
        break;
    case Reduce::hist:
        rc = hist_shape(c.prm, to.arg, &hist);
        if (rc == BSIG_OK) rc = check_params(hist.tiles, at.n, at.width, &early);
        s.cells = hist.cells;
        break;
    case Reduce::summary:
        rc = summary_shape(c.prm, to.arg, to.thresholds, &summary);
        if (rc == BSIG_OK) rc = check_params(summary.tiles, at.n, at.width, &early);
        s.row = (int64_t)summary.S * summary.row;
        s.cells = at.n * s.row;
        break;
    case Reduce::scaled:
        rc = scaled_shape(c.prm, to.arg, &scaled);
        if (rc == BSIG_OK) rc = check_params(scaled.tiles, at.n, at.width, &early);
        s.row = (int64_t)scaled.S * scaled.n_bins;
        s.cells = at.n * s.row;
        break;
    case Reduce::vplot:
        rc = vplot_shape(c.prm, at.n > 0 && at.width ? at.n : 0, at.width, to.arg, &vplot);
        s.cells = vplot.cells;
        break;
    case Reduce::capped:
        if (!to.off) return fail(BSIG_ERR_ARG, "offsets missing");
        rc = check_params(capped.tiles, at.n, at.width, &early);
        if (rc == BSIG_OK) {
            s.own_off.resize((size_t)at.n + 1);
            s.cells = bsig_layout(at.n, at.width, capped.lay_binsize, capped.S == 2, s.own_off.data());
            if (memcmp(to.off, s.own_off.data(), ((size_t)at.n + 1) * sizeof(int64_t)) != 0)
                rc = fail(BSIG_ERR_ARG, "offsets do not match bsig_layout() for these parameters");
        }
        break;
    }
    if (rc) return rc;
    if (to.reduced) std::fill(to.reduced, to.reduced + s.cells, (int64_t)0);
    if (to.kind == Reduce::capped) std::fill(to.out, to.out + s.cells, (int32_t)0);
    return BSIG_OK;
}

// Stage 2: the BAM's header and (in the background) its index.  ref: Bamfile ctor :200-214 opens file + index on every
// call; here an unchanged file (same size and mtime of the BAM and of its index) reuses the parsed header and index of
// one of the last 16 files -- keyed by the resolved path: "a.bam" and "./a.bam" are one file, one resident copy.
int open_cached_bam(Stage &s)
{
    const char *bampath = s.call.at.bampath;
    char resolved[4096];
    const std::string canon = realpath(bampath, resolved) ? std::string(resolved) : std::string(bampath);
    s.key = file_key(canon);
    s.bkey = s.key.empty() ? std::string() : s.key + "#" + index_stamps(canon);
    if (!s.bkey.empty()) {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        s.ob = Cache::touch(g_cache.bams, s.bkey);
    }
    if (s.ob) return BSIG_OK;
    bsig_bam *fresh = nullptr;
    const int rc = bam_open_lazy(bampath, &fresh);
    if (rc) return rc;
    s.ob = std::make_shared<OpenBam>();
    s.ob->key = s.bkey;
    s.ob->bam = fresh;
    if (!s.bkey.empty()) {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        g_cache.bams.push_front(s.ob);
        while (g_cache.bams.size() > 16) g_cache.bams.pop_back();
    }
    return BSIG_OK;
}

// Stage 3: seqnames -> BAM reference ids, by name (ref: parseRegions :113-120), loc = start - 1 (ref: :131); then
// bsig_plan_create's rule, before any decode, and where the result goes.
int resolve_ranges(Stage &s)
{
    const RangeArgs &at = s.call.at;
    const FileDest &to = s.call.to;
    std::vector<int32_t> level_rid((size_t)at.n_levels, -2);
    s.rid.resize((size_t)at.n);
    s.loc.resize((size_t)at.n);
    for (int64_t i = 0; i < at.n; ++i) {
        const int32_t c = at.seq_code[i];
        if (c < 0 || c >= at.n_levels) return fail(BSIG_ERR_ARG, "seqnames code %d out of range", c);
        if (level_rid[(size_t)c] == -2) level_rid[(size_t)c] = bsig_bam_name2id(s.ob->bam, at.levels[c]);
        if (level_rid[(size_t)c] < 0)
            return fail(BSIG_ERR_CHROM, "chromosome %s not present in the bam file", at.levels[c]);   // ref: :119
        s.rid[(size_t)i] = level_rid[(size_t)c];
        s.loc[(size_t)i] = at.start[i] - 1;
    }
    const int rc = check_params(s.call.prm, at.n, at.width, &s.rule, s.call.frag_len);
    if (rc) return rc;
    s.dest.flat = to.out; s.dest.off = to.off; s.dest.n = at.n;
    if (to.dst) {
        // in place: the layout is computed here
        s.own_off.resize((size_t)at.n + 1);
        bsig_layout(at.n, at.width, s.rule.lay_binsize, s.rule.ss, s.own_off.data());
        s.dest.off = s.own_off.data();
        if (s.rule.mode == BSIG_MODE_COUNT) s.dest.flat = to.dst[0]; else s.dest.ptrs = to.dst;
    }
    return BSIG_OK;
}

// ... of a gene count: the model's references are the names in `levels`; every one must be a reference of the BAM
int resolve_gene_references(Stage &s)
{
    const RangeArgs &at = s.call.at;
    s.ref_map.assign((size_t)bsig_bam_n_ref(s.ob->bam), -1);
    for (int32_t c = 0; c < at.n_levels; ++c) {
        const int32_t rid = at.levels[c] ? bsig_bam_name2id(s.ob->bam, at.levels[c]) : -1;
        if (rid < 0 || (size_t)rid >= s.ref_map.size())
            return fail(BSIG_ERR_CHROM, "chromosome %s not present in the bam file", at.levels[c] ? at.levels[c] : "(null)");
        s.ref_map[(size_t)rid] = c;
    }
    return BSIG_OK;
}

// Stage 4: the GPUs of this call.  Every device list seen keeps its own contexts, scratch and resident BAMs (a session
// that alternates between two device= arguments keeps both copies; the LRU budget bounds them).
int slots_for(const std::vector<int> &devs, Stage &s)
{
    s.rkey = s.bkey + "@";
    for (int d : devs) s.rkey += std::to_string(d) + ",";
    if (s.call.spliced) s.rkey += "|spliced";      // (a file's plain and spliced reads are two resident sets)
    if (s.call.bases) s.rkey += "|bases";          // (... and its reads with bases a third, kept only once a nucleotide call asked)
    s.many = devs.size() > 1 || env_is("BAMSIGNALS_FORCE_SHARDED", "1");     // (=1: the multi-GPU route on one GPU, testing)
    std::lock_guard<std::mutex> lock(g_cache.mu);
    for (auto &sp : g_cache.slot_sets)
        if (sp->devices == devs) s.slots = sp;
    if (s.slots) return BSIG_OK;
    auto fresh = std::make_shared<Slots>();
    fresh->devices = devs;
    for (int d : devs) {
        bsig_ctx *c = nullptr;
        const int rc = bsig_ctx_create(d, nullptr, &c);
        if (rc) return rc;
        fresh->ctx.push_back(c);
    }
    g_cache.slot_sets.push_back(fresh);
    s.slots = fresh;
    return BSIG_OK;
}

// How much of the file the ranges need, and the regions an index-driven decode would ask the index for
struct Wanted {
    bool whole = true;
    std::vector<int64_t> qbeg, qend;        // range +- ext (ref: :252-267); empty for a whole-file decode
};
// Small queries decode only the BGZF blocks the index lists (ref: one bam_itr_queryi per chunk of ranges, :252-267);
// large ones decode the whole file once and keep it in HBM for the next call.
Wanted what_to_decode(const Stage &s)
{
    const RangeArgs &at = s.call.at;
    const int64_t ext = s.rule.ext;
    int64_t genome = 0, wanted = 0;
    for (int32_t r = 0, nr = bsig_bam_n_ref(s.ob->bam); r < nr; ++r) genome += bsig_bam_ref_len(s.ob->bam, r);
    for (int64_t i = 0; i < at.n; ++i) wanted += (int64_t)at.width[i] + 2 * ext + 16384;
    const char *force = getenv("BAMSIGNALS_DECODE");   // "all" | "regions" (testing / tuning)
    // (5e7-read BAM: the whole-file decode costs 0.06-0.08 s flat and leaves the BAM resident for the
    // next call; the index-driven decode 0.02 s for 7 % of the genome, 0.09 s for 74 %)
    Wanted w;
    w.whole = wanted * 3 > genome;
    if (force && !strcmp(force, "all")) w.whole = true;
    if (force && !strcmp(force, "regions")) w.whole = false;
    if (s.call.whole_file) w.whole = true;
    if (!w.whole) {
        w.qbeg.resize((size_t)at.n); w.qend.resize((size_t)at.n);
        for (int64_t i = 0; i < at.n; ++i) {
            w.qbeg[(size_t)i] = (int64_t)s.loc[(size_t)i] - ext;
            w.qend[(size_t)i] = (int64_t)s.loc[(size_t)i] + at.width[i] + ext;
        }
    }
    return w;
}

// a whole file resident on these GPUs serves every query; failing that, an earlier index-driven decode whose regions
// contain this call's (repeated bamCount / bamProfile on the same few ranges)
bool lookup_reads(Stage &s, const Wanted &w)
{
    if (s.key.empty()) return false;
    std::lock_guard<std::mutex> lock(g_cache.mu);
    s.res = Cache::touch(g_cache.resident, s.rkey);
    s.how_decoded = s.call.spliced ? "spliced, resident" : "resident";
    if (!s.res && !w.whole) {
        s.res = Cache::touch(g_cache.regional, s.rkey, [&](const Resident &R) {
            return regions_covered(R.cov, s.call.at.n, s.rid.data(), w.qbeg.data(), w.qend.data());
        });
        s.how_decoded = s.call.spliced ? "spliced, resident (index-driven decode of an earlier call)"
                                       : "resident (index-driven decode of an earlier call)";
    }
    if (s.call.bases) s.how_decoded = "with bases, " + s.how_decoded;
    if (s.res) s.T[5] = 1;
    return s.res != nullptr;
}

// Reads onto every slot, shared by both decodes: where several slots (and the environment) allow, every GPU decodes its
// share and the column shares are all-gathered over xGMI (sharded(&transport); *transport says how, null if not taken);
// where that declines, the first GPU decodes alone (first()) and the further GPUs get device-to-device copies.
template <typename Sharded, typename First>
int decode_to_slots(Stage &s, double *t6, const char **transport, Sharded sharded, First first)
{
    Resident &R = *s.res;
    int rc = kNeedsCpuPath;
    *transport = nullptr;
    if (s.many && !env_is("BAMSIGNALS_DEVICE_DECODE", "0") && !env_is("BAMSIGNALS_SHARDED_DECODE", "0")) {
        const char *over = "";
        rc = sharded(&over);
        if (rc == BSIG_OK) *transport = over;
        bsig_device_decode_timing(t6);
    }
    if (rc == kNeedsCpuPath) {
        rc = first();
        bsig_device_decode_timing(t6);
        if (rc == BSIG_OK)
            rc = for_each_slot(R.reads.size(), [&](size_t k) -> int {
                // (a set with bases is asked on the first slot alone -- nucleotides_on_first --: its table is not copied round)
                return k == 0 || s.call.bases ? (int)BSIG_OK : bsig_reads_clone(R.reads[0], s.slots->ctx[k], &R.reads[k]);
            });
    }
    return rc;
}

// the reads file a whole-file decode may be loaded from, and is written to after the decode lock is released
struct Sidecar {
    std::string to_write, stamp;
};

// The whole file: from its reads file where there is a good one (a second process, or a call after the BAM left the cache,
// skips inflate and parse), else decoded (devdecode.hip; falls back to the CPU decode inside the call where it must).
int decode_whole(Stage &s, Sidecar &side, double *t6)
{
    const char *bampath = s.call.at.bampath;
    Resident &R = *s.res;
    const std::vector<bsig_ctx *> &ctx = s.slots->ctx;
    // (spliced reads and reads with bases have no reads file: none is loaded, none is written)
    const std::string path = s.key.empty() || s.call.spliced || s.call.bases ? std::string() : sidecar_path(bampath);
    // (the reads file is tied to the CONTENT it was made from -- size and mtime of the BAM and of its
    // index files -- not to the spelling of the path it was reached by)
    side.stamp = file_stamp(bampath) + "#" + index_stamps(bampath);
    struct stat sb;
    if (!path.empty() && stat(path.c_str(), &sb) == 0) {
        const int rc = for_each_slot(ctx.size(), [&](size_t k) { return bsig_reads_load(ctx[k], path.c_str(), side.stamp.c_str(), &R.reads[k]); });
        if (rc == BSIG_OK) {
            s.how_decoded = "sidecar";
            return BSIG_OK;
        }
        R.free_reads();
    }
    const char *transport = nullptr;
    const bool spliced = s.call.spliced, bases = s.call.bases;
    // (a spliced set is decoded on the first GPU and cloned, one with bases stays there: the sharded route declines both)
    const int rc = decode_to_slots(s, t6, &transport,
                                   [&](const char **over) { return spliced || bases ? (int)kNeedsCpuPath : reads_from_bam_sharded(ctx, bampath, 0, R.reads, over); },
                                   [&] {
                                       return bases     ? bsig_reads_from_bam_bases(ctx[0], s.ob->bam, 0, &R.reads[0])
                                              : spliced ? bsig_reads_from_bam_spliced(ctx[0], s.ob->bam, 0, &R.reads[0])
                                                        : bsig_reads_from_bam(ctx[0], s.ob->bam, 0, &R.reads[0]);
                                   });
    s.how_decoded = transport ? std::string("sharded decode, columns over ") + transport
                              : ctx.size() > 1 ? "decode on the first GPU + clones" : "decode";
    if (spliced) s.how_decoded = "spliced " + s.how_decoded;
    if (bases) s.how_decoded = "with bases, " + s.how_decoded;
    if (rc == BSIG_OK) side.to_write = path;          // written after the decode lock is released (best effort)
    return rc;
}

// Index-driven: only the blocks the index lists for the ranges (ref: one bam_itr_queryi per chunk of ranges, :252-267),
// parsed on the GPU like the whole file.  With several GPUs the islands are dealt to them (devdecode.hip).
int decode_regions(Stage &s, const Wanted &w, double *t6)
{
    bsig_bam *bam = s.ob->bam;
    Resident &R = *s.res;
    const int64_t n = s.call.at.n;
    int rc = bam_index_wait(bam);                 // (parsed in the background since the open)
    if (rc) return rc;
    const char *transport = nullptr;
    const bool spliced = s.call.spliced, bases = s.call.bases;
    rc = decode_to_slots(s, t6, &transport,
                         [&](const char **over) {
                             if (spliced || bases) return (int)kNeedsCpuPath;
                             return reads_from_regions_sharded(s.slots->ctx, s.call.at.bampath, *bsig_bam_index(bam), n, s.rid.data(),
                                                               w.qbeg.data(), w.qend.data(), 0, R.reads, over);
                         },
                         [&] {
                             if (bases)
                                 return bsig_reads_from_bam_regions_bases(s.slots->ctx[0], bam, n, s.rid.data(), w.qbeg.data(), w.qend.data(), 0,
                                                                          &R.reads[0]);
                             return spliced ? bsig_reads_from_bam_regions_spliced(s.slots->ctx[0], bam, n, s.rid.data(), w.qbeg.data(),
                                                                                 w.qend.data(), 0, &R.reads[0])
                                            : bsig_reads_from_bam_regions(s.slots->ctx[0], bam, n, s.rid.data(), w.qbeg.data(), w.qend.data(), 0,
                                                                          &R.reads[0]);
                         });
    s.how_decoded = transport ? std::string("index-driven decode, sharded, columns over ") + transport : "index-driven decode";
    if (spliced) s.how_decoded = "spliced " + s.how_decoded;
    if (bases) s.how_decoded = "with bases, " + s.how_decoded;
    if (rc == BSIG_OK) set_coverage(R.cov, n, s.rid.data(), w.qbeg.data(), w.qend.data());
    return rc;
}

// Fresh reads enter the cache.  ONE budget (env BAMSIGNALS_CACHE_GB per GPU) for whole files and index-driven decodes alike;
// above it the index-driven decodes go first, oldest first, then the least recently used whole files.  A budget of 0 keeps
// nothing but the entry in use.  Index-driven decodes: the last few (env BAMSIGNALS_REGION_CACHE, default 8; 0 = the
// reference's behaviour, none), inside the same byte budget.
void admit(const std::shared_ptr<Resident> &res, bool whole)
{
    // (what the reads hold on the device, slabs and an over-sized reservation included)
    res->bytes = res->reads[0]->pool.footprint();
    std::lock_guard<std::mutex> lock(g_cache.mu);
    bool still = false;                            // (bsig_cache_clear may have run meanwhile)
    for (auto &sp : g_cache.slot_sets) still = still || sp == res->slots;
    if (!still) return;
    const int64_t budget = cache_budget_bytes();
    if (whole) {
        for (auto it = g_cache.resident.begin(); it != g_cache.resident.end();)
            it = (*it)->key == res->key ? g_cache.resident.erase(it) : std::next(it);
        g_cache.resident.push_front(res);
    } else {
        size_t keep = 8;
        if (const char *e = getenv("BAMSIGNALS_REGION_CACHE")) keep = (size_t)std::max(0, atoi(e));
        if (budget <= 0) keep = 0;
        if (keep) g_cache.regional.push_front(res);
        while (g_cache.regional.size() > keep) g_cache.regional.pop_back();
    }
    auto held = [&]() {
        int64_t t = 0;
        for (auto &r : g_cache.resident) t += r->bytes;
        for (auto &r : g_cache.regional) t += r->bytes;
        return t;
    };
    while (held() > budget && !g_cache.regional.empty() && g_cache.regional.back() != res) g_cache.regional.pop_back();
    while (held() > budget && !g_cache.resident.empty() && g_cache.resident.back() != res) g_cache.resident.pop_back();
}

// a cold decode, under the decode lock: the reads onto every slot (once more after BSIG_ERR_NOMEM, the cache having given
// up what it can spare), the decode's timing slots, and the cache's admission
int decode_cold(Stage &s, const Wanted &w, Sidecar &side)
{
    const double t_dec = now_s();
    const AllocSnap a_dec = AllocSnap::now();
    s.res = std::make_shared<Resident>();
    s.res->key = s.rkey;
    s.res->slots = s.slots;
    s.res->reads.assign(s.slots->ctx.size(), nullptr);
    double t6[6] = {0, 0, 0, 0, 0, 0};
    int rc = BSIG_ERR_NOMEM;
    for (int attempt = 0; attempt < 2 && rc == BSIG_ERR_NOMEM; ++attempt) {
        // the cache may be what fills the device: the index-driven decodes it keeps, the result buffers of idle
        // device lists and the free blocks go back to the driver, and the decode is tried once more
        if (attempt) drop_spare_device_memory(s.slots.get());
        s.res->free_reads();
        rc = w.whole ? decode_whole(s, side, t6) : decode_regions(s, w, t6);
    }
    if (rc) return rc;
    s.T[2] = t6[5];
    s.T[1] = now_s() - t_dec - s.T[2];
    // driver allocation calls of the decode stage, layout included (they run on this thread and on the helper
    // that reserves the resident columns; the meter is per process: concurrent calls of other threads add to it)
    s.X[0] = AllocSnap::now().seconds_since(a_dec);
    decode_reservation_info(&s.X[8], &s.X[9]);
    if (!s.key.empty()) admit(s.res, w.whole);
    return BSIG_OK;
}

// Stage 5: the reads of this call on every GPU -- resident ones where the cache has them, else a cold decode in its turn
// (another thread may have decoded this very file while this one waited: a second look-up), its reads file written after
// the turn is over.
int acquire_reads(Stage &s)
{
    const Wanted w = what_to_decode(s);
    if (lookup_reads(s, w)) return BSIG_OK;
    Sidecar side;
    {
        std::unique_lock<std::mutex> turn(g_cache.decode_mu);
        if (lookup_reads(s, w)) return BSIG_OK;
        const int rc = decode_cold(s, w, side);
        if (rc) return rc;
    }
    if (!side.to_write.empty()) (void)bsig_reads_save(s.res->reads[0], side.to_write.c_str(), side.stamp.c_str());
    return BSIG_OK;
}

// The junctions of the ranges (bsig_junctions): the query of junctions.hip on the first slot's spliced set -- the table is
// the same on every slot, and only the distinct junctions come back
int junctions_on_first(const Stage &s, std::string &route)
{
    const FileCall &c = s.call;
    const RangeView g = s.ranges();
    const int rc = junctions_query(s.res->reads[0], g.n, g.rid, g.loc, g.width, g.strand, c.prm.mapqual, c.prm.requiredF, c.prm.filteredF,
                                   c.to.arg, c.prm.ss, c.to.junctions);
    route = "junctions of " + std::to_string(g.n) + " range(s), counted on the first GPU";
    return rc;
}

// The nucleotide counts of the ranges (bsig_nucleotides): the query of nucleotides.hip on the first slot's set with bases -- the
// table is the same on every slot --, downloaded into the caller's cells
int nucleotides_on_first(const Stage &s, std::string &route)
{
    const FileCall &c = s.call;
    const RangeView g = s.ranges();
    const int rc = nucleotides_query(s.res->reads[0], g.n, g.rid, g.loc, g.width, g.strand, c.prm.mapqual, c.prm.requiredF, c.prm.filteredF,
                                     c.to.arg, c.prm.ss, nullptr, c.to.out);
    route = "nucleotides of " + std::to_string(g.n) + " range(s), counted on the first GPU";
    return rc;
}

// The sites of the ranges (bsig_sites): the query of sites.hip on the first slot's set with bases, as nucleotides_on_first; only
// the sites come back
int sites_on_first(const Stage &s, std::string &route)
{
    const FileCall &c = s.call;
    const RangeView g = s.ranges();
    const int32_t *r = c.to.site_rule;
    const SiteParams prm{r[0], r[1], r[2], r[3], (uint32_t)r[4]};
    const int rc = sites_query(s.res->reads[0], g.n, g.rid, g.loc, g.width, g.strand, c.prm.mapqual, c.prm.requiredF, c.prm.filteredF, c.to.arg,
                               c.prm.ss, c.to.site_ref, prm, c.to.sites);
    route = "sites of " + std::to_string(g.n) + " range(s), found on the first GPU";
    return rc;
}

// The reads per gene (bsig_gene_counts): the query of genecounts.hip on the first slot's spliced set -- the read table is the
// same on every slot, and only the two int64 vectors come back
int gene_counts_on_first(const Stage &s, std::string &route)
{
    const FileCall &c = s.call;
    const bsig_reads *R = s.res->reads[0];
    if ((size_t)R->n_ref != s.ref_map.size()) return fail(BSIG_ERR_ARG, "the resident reads have %d references, the BAM %zu", (int)R->n_ref, s.ref_map.size());
    const int rc = gene_counts_query(R, c.to.model, s.ref_map.data(), c.prm.mapqual, c.prm.requiredF, c.prm.filteredF, c.to.arg,
                                     c.to.gene_counts, c.to.gene_summary);
    route = "gene counts of " + std::to_string(c.to.model->host.n_genes) + " gene(s), counted on the first GPU";
    return rc;
}

// one GPU, the per-range result: plan (ranges -> tiles in HBM), kernels, download -- timed apart
int run_on_one(const Stage &s, double t_run)
{
    const int64_t n = s.call.at.n;
    bsig_plan *plan = nullptr;
    int rc = plain_plan(s.slots->ctx[0], s.res->reads[0], s.ranges(), s.call, &plan);
    s.X[3] = now_s() - t_run;
    if (rc == BSIG_OK && memcmp(s.dest.off, bsig_plan_offsets(plan), (size_t)(n + 1) * sizeof(int64_t)) != 0)
        rc = fail(BSIG_ERR_ARG, "offsets do not match bsig_layout() for these parameters");
    if (rc == BSIG_OK) rc = plan_run_to_host(plan, &s.dest, false, &s.X[4], &s.X[5]);
    if (plan) bsig_plan_free(plan);
    return rc;
}

// Stage 6: the result by the call's shape; out of device memory, once more with the cache's spare memory given back.
// `result` receives the route's words.
int run_result(const Stage &s, std::string &result)
{
    const FileDest &to = s.call.to;
    const double t_run = now_s();
    int rc = BSIG_ERR_NOMEM;
    for (int attempt = 0; attempt < 2 && rc == BSIG_ERR_NOMEM; ++attempt) {
        if (attempt) drop_spare_device_memory(s.slots.get());
        if (to.shape == FileDest::Shape::junctions) rc = junctions_on_first(s, result);
        else if (to.shape == FileDest::Shape::genes) rc = gene_counts_on_first(s, result);
        else if (to.shape == FileDest::Shape::nucleotides) rc = nucleotides_on_first(s, result);
        else if (to.shape == FileDest::Shape::sites) rc = sites_on_first(s, result);
        else if (to.shape == FileDest::Shape::reduced) rc = reduced_on_slots(s, result);
        else if (to.runs) rc = encoded_on_slots(s, result);
        else if (!s.many) rc = run_on_one(s, t_run);
        else rc = run_on_slots(s, result);
    }
    if (!s.many && to.shape != FileDest::Shape::reduced && to.shape != FileDest::Shape::junctions && to.shape != FileDest::Shape::genes &&
        to.shape != FileDest::Shape::nucleotides && to.shape != FileDest::Shape::sites && !to.runs)
        result = "download";
    return rc;
}

}  // namespace

int scatter_segments_to(int64_t n, const int32_t *src, const int64_t *src_off, const HostDest &dst, const int64_t *which)
{
    if (n > 0 && (!src_off || !dst.off || !which)) return fail(BSIG_ERR_ARG, "NULL argument");
    for (int64_t k = 0; k < n; ++k) {
        const int64_t len = src_off[k + 1] - src_off[k];
        const int64_t i = which[k];
        if (len < 0 || i < 0) return fail(BSIG_ERR_ARG, "bad segment %lld", (long long)k);
        if (len != dst.off[i + 1] - dst.off[i]) return fail(BSIG_ERR_ARG, "segment %lld does not fit its destination", (long long)k);
    }
    if (n <= 0) return BSIG_OK;
    auto copy_range = [&](int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t len = src_off[k + 1] - src_off[k];
            if (len) memcpy(dst.range(which[k]), src + src_off[k], (size_t)len * sizeof(int32_t));
        }
    };
    // the destinations are disjoint (each range owns its cells): big results are moved by a few
    // threads, each taking a contiguous share of the source
    const int64_t cells = src_off[n] - src_off[0];
    int n_thr = cells * (int64_t)sizeof(int32_t) >= (16 << 20) ? 8 : 1;
    if (const char *e = getenv("BAMSIGNALS_COPY_THREADS")) n_thr = std::max(1, std::min(64, atoi(e)));
    n_thr = (int)std::min<int64_t>(n_thr, n);
    if (n_thr <= 1) { copy_range(0, n); return BSIG_OK; }
    std::vector<int64_t> cut((size_t)n_thr + 1, n);
    cut[0] = 0;
    for (int t = 1; t < n_thr; ++t) {
        const int64_t target = src_off[0] + cells * t / n_thr;
        cut[(size_t)t] = std::lower_bound(src_off, src_off + n, target) - src_off;
    }
    std::vector<std::thread> th;
    for (int t = 1; t < n_thr; ++t) th.emplace_back(copy_range, cut[(size_t)t], cut[(size_t)t + 1]);
    copy_range(cut[0], cut[1]);
    for (auto &x : th) x.join();
    return BSIG_OK;
}

// One file-level call: the stages in order, the timing slots around them, the route at the end.
int file_level(const FileCall &call)
{
    double *T = g_call_timing, *X = g_call_timing_ex;
    Stage s{call, T, X};
    int rc = judge_call(call, s);
    if (rc) return rc;
    for (int k = 0; k < 6; ++k) T[k] = 0;
    for (int k = 0; k < 10; ++k) X[k] = 0;
    const double t_begin = now_s();
    const AllocSnap a_begin = AllocSnap::now();
    rc = open_cached_bam(s);
    if (rc) return rc;
    T[0] = now_s() - t_begin;
    rc = resolve_ranges(s);
    if (rc == BSIG_OK && call.to.shape == FileDest::Shape::genes) rc = resolve_gene_references(s);
    if (rc == BSIG_OK) rc = slots_for(pick_devices(call.device), s);
    if (rc == BSIG_OK) rc = acquire_reads(s);
    if (rc) return rc;
    const double t_run = now_s();
    const AllocSnap a_run = AllocSnap::now();
    std::string result;
    rc = run_result(s, result);
    T[3] = now_s() - t_run;
    const AllocSnap a_end = AllocSnap::now();
    X[1] = a_end.seconds_since(a_run);
    X[2] = a_end.seconds_since(a_begin);
    X[6] = (double)(a_end.calls - a_begin.calls);
    if (rc == BSIG_OK) rc = bam_index_wait(s.ob->bam);      // a damaged index fails the call, as it does in the reference's open
    T[4] = now_s() - t_begin;
    snprintf(g_call_route, sizeof g_call_route, "%zu GPU slot(s); reads: %s; result: %s", s.slots->devices.size(), s.how_decoded.c_str(),
             result.c_str());
    return rc;
}

}  // namespace bsig

using bsig::g_cache;
extern "C" {

void bsig_last_call_timing(double *t6)
{
    for (int k = 0; k < 6; ++k) t6[k] = bsig::g_call_timing[k];
}

void bsig_last_call_timing_ex(double *t, int32_t n)
{
    for (int k = 0; k < n && k < 16; ++k) t[k] = k < 6 ? bsig::g_call_timing[k] : bsig::g_call_timing_ex[k - 6];
}

const char *bsig_last_call_route(void) { return bsig::g_call_route; }

void bsig_cache_clear(void)
{
    // everything is moved out under the lock and released outside it (freeing HBM takes a while); what a
    // running call holds -- its contexts, scratch, resident reads, communicators -- lives until it returns
    bsig::Cache old;
    {
        std::lock_guard<std::mutex> lock(g_cache.mu);
        old.resident.swap(g_cache.resident);
        old.regional.swap(g_cache.regional);
        old.bams.swap(g_cache.bams);
        old.slot_sets.swap(g_cache.slot_sets);
    }
    old.clear();
    bsig::exchange_close_all();
    bsig::release_decode_scratch();
}

int64_t bsig_debug_scratch_allocs(void)
{
    // allocations made so far for the multi-GPU result path's cached buffers (tests: flat across resident calls)
    std::lock_guard<std::mutex> lock(g_cache.mu);
    int64_t n = 0;
    for (auto &sp : g_cache.slot_sets) n += sp->scratch_allocs.load();
    return n;
}

}  // extern "C"
