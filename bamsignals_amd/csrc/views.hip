// Views of int32 device buffers (bsig_views_*): the stretches of a per-range result whose cells lie in [lower, upper],
// each with its sum, its max and its summit -- IRanges' slice() with viewSums / viewMaxs / viewWhichMaxs, the callable
// regions of a depth threshold, the candidate peaks of a pileup -- without the per-base cells ever leaving HBM.
//
// The input is runs.hip's: any int32 device buffer plus a table of SEGMENTS (encode_common.h).  A cell is IN iff
// lower <= v <= upper (signed); a VIEW is a maximal stretch of consecutive in-cells of one segment, so a segment boundary
// always ends a view.  The flattened cell space is cut into stretches of `chunk` cells, a workgroup is ONE wave and takes
// one stretch; passes with launch boundaries between them (no workgroup ever waits for another one):
//   1. k_views_walk<false>  counts the view starts of every stretch (a cell is a start iff it is in, and it is first in
//                           its segment or its predecessor is not in): per 64 cells one __ballot of the in-cells, one of
//                           the segments' first cells, a shift and one population count
//   2. k_runs_scan          (encode_common.h) exclusive scan of the stretch counts in 64 bits, and the total
//      -- the host reads the total, allocates start / width / sum / max / summit at their exact size and zeroes width,
//         sum and the summit keys --
//   3. k_views_walk<true>   the same walk: every start stores its cell index at its scanned slot, the first cell of a
//                           segment stores the starts before it as the segment's view offset.  Per 64 cells the in-cells
//                           are reduced per view by a segmented scan across the lanes to a width, a 64-bit sum and a KEY
//                              (uint64)(v ^ 0x80000000) << 32 | (0xFFFFFFFF - cell index in segment)
//                           whose maximum is the largest value and, among equal values, the leftmost cell.  A view that
//                           begins and ends inside one round of 64 cells is stored by its last lane.  A view that
//                           reaches a round's last lane is carried in wave-uniform registers into the next round and
//                           flushed where it ends: with plain stores when it began and ended inside the stretch, else --
//                           it crosses a seam, or touches the stretch's last cell -- with integer atomics (add on width
//                           and sum, max on the key) into the zeroed slot.  A stretch whose first cell continues a view
//                           of the stretch before it adds to slot st_base - 1: that view's start is the last start in
//                           front of the stretch.  Integer adds and a max commute: the result is the same on every run.
//      k_views_unpack       max and summit out of the key
//      k_runs_fill_empty    (encode_common.h) view offsets of zero-length segments (only if the table has any)
// The predecessor of a lane's cell is its neighbour's bit of the ballot; that of a round's first cell is the top bit
// of the round before, and that of a stretch's first cell is read from global memory.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/bamsignals_abi.h"
#include "encode_common.h"
#include "host_util.h"
#include "runtime_internal.h"

using bsig::fail;

namespace {

constexpr int kUnroll = 4;                   // rounds of 64 cells whose loads are issued together

__device__ __forceinline__ uint64_t view_key(int32_t v, uint32_t p)
{
    return ((uint64_t)((uint32_t)v ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - p);
}

// one view's partial result of one stretch into its slot: plain stores where no other stretch touches the slot
__device__ __forceinline__ void view_flush(bool plain, int64_t r, int64_t n_views, uint32_t cnt, int64_t sum, uint64_t key,
                                           int32_t *__restrict__ width, int64_t *__restrict__ sums, uint64_t *__restrict__ keys)
{
    if (r < 0 || r >= n_views) return;      // (a buffer that changed between the walks: never out of bounds)
    if (plain) {
        width[r] = (int32_t)cnt;
        sums[r] = sum;
        keys[r] = key;
    } else {
        atomicAdd((unsigned int *)&width[r], cnt);
        atomicAdd((unsigned long long *)&sums[r], (unsigned long long)sum);
        atomicMax((unsigned long long *)&keys[r], (unsigned long long)key);
    }
}

// EMIT = false: counts[stretch] = view starts of the stretch.  EMIT = true: st_base[stretch] = views before the stretch;
// start / width / sums / keys at the views' slots, seg_off at a segment's first cell.
template <bool EMIT>
__global__ __launch_bounds__(kWave) void k_views_walk(const int32_t *__restrict__ src, const int64_t *__restrict__ cell0,
                                                      const int64_t *__restrict__ base, int64_t n_seg, int32_t stride,
                                                      int64_t total, int32_t chunk, int32_t lower, int32_t upper,
                                                      uint32_t *__restrict__ counts, const int64_t *__restrict__ st_base,
                                                      int64_t n_views, int32_t *__restrict__ start, int32_t *__restrict__ width,
                                                      int64_t *__restrict__ sums, uint64_t *__restrict__ keys,
                                                      int64_t *__restrict__ seg_off)
{
    const int lane = threadIdx.x;
    const int64_t c_begin = (int64_t)blockIdx.x * chunk;
    if (c_begin >= total) return;
    const int64_t c_end = c_begin + chunk < total ? c_begin + chunk : total;
    // the stretch's first and last segment (the same for all lanes)
    const int64_t s_lo = seg_of(cell0, 0, n_seg - 1, c_begin);
    const int64_t s_hi = seg_of(cell0, s_lo, n_seg - 1, c_end - 1);
    const bool one_seg = s_lo == s_hi;
    const int64_t cell0_lo = cell0[s_lo], base_lo = base[s_lo];
    // is the cell in front of the stretch in, where it belongs to the stretch's first segment?
    uint64_t carry = 0;
    if (c_begin > cell0_lo) {
        const int32_t v = src[base_lo + (c_begin - 1 - cell0_lo) * stride];
        carry = v >= lower && v <= upper;
    }
    int64_t s = s_lo;                                   // this lane's segment: never decreases
    int64_t slot = EMIT ? st_base[blockIdx.x] : 0;      // starts in front of the round
    uint32_t n_starts = 0;
    const uint64_t below = ((uint64_t)1 << lane) - 1, upto = below | ((uint64_t)1 << lane);
    // the view that reached the last lane of the round before (wave-uniform)
    bool open = false, o_plain = false;
    uint32_t o_cnt = 0;
    int64_t o_sum = 0, o_slot = 0;
    uint64_t o_key = 0;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += (int64_t)kUnroll * kWave) {
        int32_t v[kUnroll];
        bool valid[kUnroll], first[kUnroll];
        int64_t seg[kUnroll];
        uint32_t p32[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t c = c0 + u * kWave + lane;
            valid[u] = c < c_end;
            v[u] = 0;
            first[u] = false;
            seg[u] = s;
            p32[u] = 0;
            if (valid[u]) {
                int64_t p, b;
                if (one_seg) {
                    p = c - cell0_lo;
                    b = base_lo;
                } else {
                    s = seg_of(cell0, s, s_hi, c);
                    p = c - cell0[s];
                    b = base[s];
                }
                seg[u] = s;
                first[u] = p == 0;
                p32[u] = (uint32_t)p;
                v[u] = src[b + p * stride];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t cr = c0 + u * kWave;          // the round's first cell
            if (cr >= c_end) break;
            const bool in = valid[u] && v[u] >= lower && v[u] <= upper;
            const uint64_t inmask = __ballot(in);
            const uint64_t firstmask = __ballot(first[u]);
            const uint64_t startmask = inmask & (firstmask | ~((inmask << 1) | carry));
            carry = inmask >> (kWave - 1);
            if (!EMIT) {
                n_starts += (uint32_t)__popcll(startmask);
                continue;
            }
            const int n_before = __popcll(startmask & below);
            if (first[u] && valid[u]) seg_off[seg[u]] = slot + n_before;
            if (inmask == 0) {
                if (open) {         // it ended with the round before
                    if (lane == 0) view_flush(o_plain, o_slot, n_views, o_cnt, o_sum, o_key, width, sums, keys);
                    open = false;
                }
                continue;
            }
            const bool is_start = (startmask >> lane) & 1;
            if (is_start && slot + n_before < n_views) start[slot + n_before] = (int32_t)p32[u];
            // the round's last cell, and the lanes that end a view inside the round
            const int last = c_end - cr < kWave ? (int)(c_end - cr) - 1 : kWave - 1;
            const uint64_t endmask = inmask & ~((inmask & ~startmask) >> 1);
            // this lane's view begins at lane `head` (0: it came in from the round before)
            const uint64_t heads = startmask & upto;
            const int head = heads ? 63 - __clzll((long long)heads) : 0;
            // inclusive segmented scan of sum and key across the lanes of a view (a step that no lane takes ends it)
            int64_t sum = in ? (int64_t)v[u] : 0;
            uint64_t key = in ? view_key(v[u], p32[u]) : 0;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const bool take = in && lane - d >= head;
                if (__ballot(take) == 0) break;
                const int64_t s_up = __shfl_up(sum, d);
                const uint64_t k_up = __shfl_up(key, d);
                if (take) {
                    sum += s_up;
                    key = k_up > key ? k_up : key;
                }
            }
            const bool cont = (inmask & 1) && !(startmask & 1);     // lane 0 continues a view
            int e0 = -1;                                            // ... which ends at lane e0
            if (cont) {
                e0 = __ffsll((unsigned long long)endmask) - 1;
                if (!open) {        // (the stretch's first round: the view of the stretch before)
                    open = true;
                    o_plain = false;
                    o_cnt = 0; o_sum = 0; o_key = 0;
                    o_slot = slot - 1;
                }
                const int64_t s_e = __shfl(sum, e0);
                const uint64_t k_e = __shfl(key, e0);
                o_cnt += (uint32_t)e0 + 1;
                o_sum += s_e;
                o_key = k_e > o_key ? k_e : o_key;
            }
            if (open && !(cont && e0 == last)) {        // the carried view ends inside this stretch
                if (lane == 0) view_flush(o_plain, o_slot, n_views, o_cnt, o_sum, o_key, width, sums, keys);
                open = false;
            }
            // the views that begin in this round ...
            const int n_upto = __popcll(heads);
            const bool ends_here = ((endmask >> lane) & 1) && n_upto > 0;
            if (ends_here && lane != last)              // ... and end in it
                view_flush(true, slot + n_upto - 1, n_views, (uint32_t)(lane - head + 1), sum, key, width, sums, keys);
            if (((inmask >> last) & 1) && !(cont && e0 == last)) {      // ... and reach its last cell: carried on
                const int n_all = __popcll(startmask);
                const uint64_t h_all = startmask;                       // (not empty: the view began in this round)
                const int head_l = 63 - __clzll((long long)h_all);
                open = true;
                o_plain = true;
                o_cnt = (uint32_t)(last - head_l + 1);
                o_sum = __shfl(sum, last);
                o_key = __shfl(key, last);
                o_slot = slot + n_all - 1;
            }
            slot += __popcll(startmask);
        }
    }
    if (!EMIT) {
        if (lane == 0) counts[blockIdx.x] = n_starts;
        return;
    }
    // the view that touches the stretch's last cell may go on in the next stretch
    if (open && lane == 0) view_flush(false, o_slot, n_views, o_cnt, o_sum, o_key, width, sums, keys);
}

__global__ __launch_bounds__(kFlatThreads) void k_views_unpack(int64_t n_views, const uint64_t *__restrict__ keys,
                                                               int32_t *__restrict__ max, int32_t *__restrict__ summit)
{
    const int64_t r = (int64_t)blockIdx.x * kFlatThreads + threadIdx.x;
    if (r >= n_views) return;
    const uint64_t k = keys[r];
    max[r] = (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u);
    summit[r] = (int32_t)(0xFFFFFFFFu - (uint32_t)k);
}

}  // namespace

// (the segment table and the scan's arrays: encode_common.h)
struct bsig_views : SegTable {
    std::unique_ptr<DevPool> res;        // the five value arrays of the last encode, at their exact size
    int64_t n_views = -1;                // of the last encode (-1: none yet)
    int32_t *start = nullptr, *width = nullptr, *max = nullptr, *summit = nullptr;
    int64_t *sum = nullptr;
};

extern "C" {

int bsig_views_create(bsig_ctx *ctx, int64_t n_seg, const int64_t *base, const int32_t *len, int32_t stride, bsig_views **out)
{
    if (!ctx || !out) return fail(BSIG_ERR_ARG, "NULL argument");
    *out = nullptr;
    std::unique_ptr<bsig_views> V(new bsig_views);
    if (const int rc = V->build(ctx, n_seg, base, len, stride, "BAMSIGNALS_VIEWS_CHUNK_CELLS")) return rc;
    *out = V.release();
    return BSIG_OK;
}

int64_t bsig_views_n_seg(const bsig_views *V) { return V ? V->n_seg : 0; }

int64_t bsig_views_cells(const bsig_views *V) { return V ? V->total : 0; }

int bsig_views_encode(bsig_views *V, const int32_t *src_dev, int32_t lower, int32_t upper, int64_t *n_views)
{
    if (!V) return fail(BSIG_ERR_ARG, "views is NULL");
    if (lower > upper) return fail(BSIG_ERR_ARG, "lower (%d) is above upper (%d)", (int)lower, (int)upper);
    if (V->total > 0 && !src_dev) return fail(BSIG_ERR_ARG, "source buffer is NULL");
    HIP_TRY(hipSetDevice(V->ctx->device));
    hipStream_t st = V->ctx->stream;
    V->n_views = -1;
    V->start = V->width = V->max = V->summit = nullptr;
    V->sum = nullptr;
    V->res.reset();
    int64_t total_views = 0;
    if (V->total > 0) {
        hipLaunchKernelGGL(k_views_walk<false>, dim3((unsigned)V->n_st), dim3(kWave), 0, st, src_dev, V->cell0, V->base, V->n_seg,
                           V->stride, V->total, V->chunk, lower, upper, V->counts, nullptr, (int64_t)0, nullptr, nullptr, nullptr, nullptr,
                           nullptr);
        hipLaunchKernelGGL(k_runs_scan, dim3(1), dim3(kScanThreads), 0, st, V->n_st, V->counts, V->st_base, V->d_total);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&total_views, V->d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // (a view has a cell of its own: segments of one in-cell each are as many views as cells)
        if (total_views < 0 || total_views > V->total) return fail(BSIG_ERR_DEVICE, "view count %lld out of range", (long long)total_views);
    }
    if (total_views > 0) {
        const size_t n = (size_t)total_views;
        // sum, the summit keys and width in one block: one memset zeroes what the seams add into (the keys stay with the
        // result until the next encode)
        int64_t *zeroed = nullptr;
        V->res.reset(new DevPool);
        HIP_TRY(V->res->alloc(&V->start, n));
        HIP_TRY(V->res->alloc(&zeroed, 2 * n + (n + 1) / 2));
        HIP_TRY(V->res->alloc(&V->max, n));
        HIP_TRY(V->res->alloc(&V->summit, n));
        V->sum = zeroed;
        uint64_t *keys = (uint64_t *)(zeroed + n);
        V->width = (int32_t *)(zeroed + 2 * n);
        HIP_TRY(hipMemsetAsync(zeroed, 0, (2 * n + (n + 1) / 2) * sizeof(int64_t), st));
        hipLaunchKernelGGL(k_views_walk<true>, dim3((unsigned)V->n_st), dim3(kWave), 0, st, src_dev, V->cell0, V->base, V->n_seg,
                           V->stride, V->total, V->chunk, lower, upper, nullptr, V->st_base, total_views, V->start, V->width, V->sum, keys,
                           V->seg_off);
        hipLaunchKernelGGL(k_views_unpack, dim3((unsigned)((total_views + kFlatThreads - 1) / kFlatThreads)), dim3(kFlatThreads), 0, st,
                           total_views, keys, V->max, V->summit);
        if (V->has_empty) {
            hipLaunchKernelGGL(k_runs_fill_empty, dim3((unsigned)((V->n_seg + 1 + kFlatThreads - 1) / kFlatThreads)), dim3(kFlatThreads), 0,
                               st, V->n_seg, V->cell0, V->total, total_views, V->seg_off);
        } else {
            HIP_TRY(hipMemcpyAsync(V->seg_off + V->n_seg, V->d_total, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(hipGetLastError());
    } else {
        // no view: every segment owns none
        HIP_TRY(hipMemsetAsync(V->seg_off, 0, ((size_t)V->n_seg + 1) * sizeof(int64_t), st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    V->n_views = total_views;
    if (n_views) *n_views = total_views;
    return BSIG_OK;
}

int bsig_views_device(const bsig_views *V, int64_t *n_views, const int64_t **seg_off, const int32_t **start, const int32_t **width,
                      const int64_t **sum, const int32_t **max, const int32_t **summit)
{
    if (!V) return fail(BSIG_ERR_ARG, "views is NULL");
    if (V->n_views < 0) return fail(BSIG_ERR_ARG, "nothing has been encoded yet");
    if (n_views) *n_views = V->n_views;
    if (seg_off) *seg_off = V->seg_off;
    if (start) *start = V->start;
    if (width) *width = V->width;
    if (sum) *sum = V->sum;
    if (max) *max = V->max;
    if (summit) *summit = V->summit;
    return BSIG_OK;
}

int bsig_views_fetch(bsig_views *V, int64_t *seg_off, int32_t *start, int32_t *width, int64_t *sum, int32_t *max, int32_t *summit)
{
    if (!V) return fail(BSIG_ERR_ARG, "views is NULL");
    if (V->n_views < 0) return fail(BSIG_ERR_ARG, "nothing has been encoded yet");
    if (!seg_off || (V->n_views > 0 && (!start || !width || !sum || !max || !summit))) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    HIP_TRY(hipSetDevice(V->ctx->device));
    const size_t n = (size_t)V->n_views;
    int rc = bsig::download_to_host(V->ctx, V->seg_off, seg_off, ((size_t)V->n_seg + 1) * sizeof(int64_t));
    if (rc == BSIG_OK && n) rc = bsig::download_to_host(V->ctx, V->start, start, n * sizeof(int32_t));
    if (rc == BSIG_OK && n) rc = bsig::download_to_host(V->ctx, V->width, width, n * sizeof(int32_t));
    if (rc == BSIG_OK && n) rc = bsig::download_to_host(V->ctx, V->sum, sum, n * sizeof(int64_t));
    if (rc == BSIG_OK && n) rc = bsig::download_to_host(V->ctx, V->max, max, n * sizeof(int32_t));
    if (rc == BSIG_OK && n) rc = bsig::download_to_host(V->ctx, V->summit, summit, n * sizeof(int32_t));
    return rc;
}

void bsig_views_free(bsig_views *V)
{
    if (!V) return;
    (void)hipSetDevice(V->ctx->device);
    delete V;
}

}  // extern "C"
