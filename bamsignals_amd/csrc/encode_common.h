// What the device encoders of int32 buffers share (runs.hip: bsig_runs_*, views.hip: bsig_views_*): the table of
// SEGMENTS on the device, the binary search of a flattened cell's segment, the scan of the stretch counts and the
// offsets of the segments without cells.  Kernels are local to the file that includes this (no relocatable device code).
//
// Segment k is the len[k] cells src[base[k] + p * stride], p = 0 .. len[k] - 1.  The segments laid behind each other are
// the FLATTENED cell space (cell0[k] = len[0] + .. + len[k - 1]), cut by cells into stretches of `chunk` cells; a
// workgroup is ONE wave and takes one stretch.
#ifndef BSIG_ENCODE_COMMON_H
#define BSIG_ENCODE_COMMON_H
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "../../include/bamsignals_abi.h"
#include "host_util.h"
#include "runtime_internal.h"

namespace {

constexpr int kWave = 64;
constexpr int kScanThreads = 1024;
constexpr int kFlatThreads = 256;            // the per-result and per-segment passes
constexpr int32_t kDefaultChunk = 2048;      // cells per stretch (env BAMSIGNALS_RUNS_CHUNK_CELLS / BAMSIGNALS_VIEWS_CHUNK_CELLS)

// the segment of flattened cell c: the largest s in [lo, hi] with cell0[s] <= c (cell0[lo] <= c; empty segments share
// their cell0 with the next segment, so the largest one is the segment that holds the cell)
__device__ __forceinline__ int64_t seg_of(const int64_t *__restrict__ cell0, int64_t lo, int64_t hi, int64_t c)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (cell0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Exclusive scan of the stretch counts in 64 bits, and the total.  One workgroup, as k_chunk_scan (kernels.hip): every
// thread sums a slab of consecutive stretches, the slab sums are scanned in LDS, every thread writes its slab's bases.
__global__ __launch_bounds__(kScanThreads) void k_runs_scan(int64_t n, const uint32_t *__restrict__ counts,
                                                            int64_t *__restrict__ st_base, int64_t *__restrict__ total)
{
    __shared__ int64_t slab[kScanThreads];
    const int tid = threadIdx.x;
    const int64_t per = (n + kScanThreads - 1) / kScanThreads;
    const int64_t k0 = (int64_t)tid * per < n ? (int64_t)tid * per : n, k1 = k0 + per < n ? k0 + per : n;
    int64_t sum = 0;
    for (int64_t k = k0; k < k1; ++k) sum += counts[k];
    slab[tid] = sum;
    __syncthreads();
    // inclusive scan over the slabs, in place (Hillis-Steele: ten steps)
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int64_t add = tid >= d ? slab[tid - d] : 0;
        __syncthreads();
        slab[tid] += add;
        __syncthreads();
    }
    int64_t run = slab[tid] - sum;
    for (int64_t k = k0; k < k1; ++k) {
        st_base[k] = run;
        run += counts[k];
    }
    if (tid == kScanThreads - 1) *total = slab[tid];
}

// seg_off of the zero-length segments and seg_off[n_seg]: a zero-length segment has the offset of the next segment
// that holds a cell (which the emitting walk stored), or the total
__global__ __launch_bounds__(kFlatThreads) void k_runs_fill_empty(int64_t n_seg, const int64_t *__restrict__ cell0, int64_t total,
                                                                  int64_t n_runs, int64_t *__restrict__ seg_off)
{
    const int64_t k = (int64_t)blockIdx.x * kFlatThreads + threadIdx.x;
    if (k > n_seg) return;
    if (k == n_seg) { seg_off[k] = n_runs; return; }
    const int64_t c = cell0[k];
    if (cell0[k + 1] != c) return;
    seg_off[k] = c >= total ? n_runs : seg_off[seg_of(cell0, k, n_seg - 1, c)];
}

// The segment table of an encoder on its device, and the arrays of the count-and-scan passes: as long as the object.
struct SegTable {
    bsig_ctx *ctx = nullptr;
    int64_t n_seg = 0, total = 0, n_st = 0;
    int32_t stride = 1, chunk = kDefaultChunk;
    bool has_empty = false;
    DevPool pool;
    int64_t *cell0 = nullptr;            // n_seg + 1
    int64_t *base = nullptr;             // n_seg
    uint32_t *counts = nullptr;          // n_st
    int64_t *st_base = nullptr;          // n_st
    int64_t *d_total = nullptr;
    int64_t *seg_off = nullptr;          // n_seg + 1

    // checks the table (BSIG_ERR_ARG), reads the chunk knob `chunk_env` (64 .. 2^24), uploads; synchronises
    int build(bsig_ctx *c, int64_t n, const int64_t *base_host, const int32_t *len, int32_t stride_, const char *chunk_env)
    {
        using bsig::fail;
        if (n < 0) return fail(BSIG_ERR_ARG, "negative number of segments");
        if (n > 0 && (!base_host || !len)) return fail(BSIG_ERR_ARG, "segment table missing");
        if (stride_ != 1 && stride_ != 2) return fail(BSIG_ERR_ARG, "stride must be 1 or 2");
        std::vector<int64_t> c0((size_t)n + 1);
        int64_t acc = 0;
        for (int64_t k = 0; k < n; ++k) {
            if (len[k] < 0) return fail(BSIG_ERR_ARG, "segment %lld has a negative length", (long long)k);
            if (base_host[k] < 0) return fail(BSIG_ERR_ARG, "segment %lld has a negative base", (long long)k);
            c0[(size_t)k] = acc;
            acc += len[k];
            has_empty = has_empty || len[k] == 0;
        }
        c0[(size_t)n] = acc;
        ctx = c;
        n_seg = n;
        total = acc;
        stride = stride_;
        if (const char *e = getenv(chunk_env)) {      // (testing: seams everywhere)
            const long long v = atoll(e);
            if (v >= kWave && v <= (1 << 24)) chunk = (int32_t)v;
        }
        n_st = (acc + chunk - 1) / chunk;
        if (n_st > INT32_MAX) return fail(BSIG_ERR_ARG, "too many cells for one encoder: %lld", (long long)acc);
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        HIP_TRY(pool.alloc(&cell0, (size_t)n + 1));
        HIP_TRY(pool.alloc(&seg_off, (size_t)n + 1));
        HIP_TRY(pool.alloc(&d_total, 1));
        HIP_TRY(hipMemcpyAsync(cell0, c0.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (n) {
            HIP_TRY(pool.alloc(&base, (size_t)n));
            HIP_TRY(hipMemcpyAsync(base, base_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        }
        if (n_st) {
            HIP_TRY(pool.alloc(&counts, (size_t)n_st));
            HIP_TRY(pool.alloc(&st_base, (size_t)n_st));
        }
        HIP_TRY(hipStreamSynchronize(st));      // (the host tables go away)
        return BSIG_OK;
    }
};

}  // namespace
#endif
