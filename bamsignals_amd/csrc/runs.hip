// Run-length encoding of int32 device buffers (bsig_runs_*): the per-range result as (value, length) runs, the form an
// Rle / a bedGraph has, without the per-base cells ever leaving HBM.
//
// The input is any int32 device buffer plus a table of SEGMENTS: segment k is the len[k] cells src[base[k] + p * stride],
// p = 0 .. len[k] - 1 (stride 1, or 2 for one row of the interleaved 2 * bin + antisense layout).  The runs of a
// segment are its maximal stretches of equal consecutive cells; a segment boundary always starts a run.
//
// The segments laid behind each other are the FLATTENED cell space (cell0[k] = len[0] + .. + len[k - 1]).  It is cut by
// cells, not by segments, into stretches of `chunk` cells; a workgroup is ONE wave and takes one stretch -- a piece of a
// 250-Mbp segment or several thousand whole 200-bp segments cost the same.  Three passes with launch boundaries between
// them (no workgroup ever waits for another one):
//   1. k_runs_walk<false>  counts the run starts of every stretch (a cell is a start iff it is first in its segment or
//                          differs from its predecessor): one __ballot and one population count per 64 cells
//   2. k_runs_scan         one workgroup: exclusive scan of the stretch counts in 64 bits, and the total (encode_common.h,
//                          with the segment table, seg_of and k_runs_fill_empty: shared with views.hip)
//      -- the host reads the total and allocates values / lengths / positions at their exact size --
//   3. k_runs_walk<true>   the same walk: every start stores its value and its flattened position at its scanned slot;
//                          the first cell of a segment also stores its slot as the segment's run offset
//      k_runs_lengths      length[r] = position[r + 1] - position[r] (the flattened space has no gaps and every segment
//                          begins with a start, so the next start IS this run's end, across segments as well)
//      k_runs_fill_empty   run offsets of zero-length segments (only if the table has any)
// The predecessor of a lane's cell is its neighbour lane's cell (one shuffle); that of a wave's first cell is the last
// lane's cell of the round before, and that of a stretch's first cell is read from global memory.
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

// EMIT = false: counts[stretch] = run starts of the stretch.  EMIT = true: st_base[stretch] = runs before the stretch;
// every start stores values / pos at its slot, a segment's first cell stores seg_off.
template <bool EMIT>
__global__ __launch_bounds__(kWave) void k_runs_walk(const int32_t *__restrict__ src, const int64_t *__restrict__ cell0,
                                                     const int64_t *__restrict__ base, int64_t n_seg, int32_t stride,
                                                     int64_t total, int32_t chunk, uint32_t *__restrict__ counts,
                                                     const int64_t *__restrict__ st_base, int32_t *__restrict__ values,
                                                     uint32_t *__restrict__ pos, int64_t *__restrict__ seg_off)
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
    // the cell in front of the stretch, where it belongs to the stretch's first segment
    int32_t carry = 0;
    if (c_begin > cell0_lo) carry = src[base_lo + (c_begin - 1 - cell0_lo) * stride];
    int64_t s = s_lo;                                   // this lane's segment: never decreases
    int64_t slot = EMIT ? st_base[blockIdx.x] : 0;      // runs in front of the round
    uint32_t n_starts = 0;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += (int64_t)kUnroll * kWave) {
        int32_t v[kUnroll];
        bool valid[kUnroll], first[kUnroll];
        int64_t seg[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t c = c0 + u * kWave + lane;
            valid[u] = c < c_end;
            v[u] = 0;
            first[u] = false;
            seg[u] = s;
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
                v[u] = src[b + p * stride];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            int32_t prev = __shfl_up(v[u], 1);
            if (lane == 0) prev = carry;
            carry = __shfl(v[u], kWave - 1);
            const bool start = valid[u] && (first[u] || v[u] != prev);
            const uint64_t mask = __ballot(start);
            if (EMIT) {
                if (start) {
                    const int64_t r = slot + __popcll(mask & below);
                    values[r] = v[u];
                    pos[r] = (uint32_t)(c0 + u * kWave + lane);
                    if (first[u]) seg_off[seg[u]] = r;
                }
                slot += __popcll(mask);
            } else {
                n_starts += (uint32_t)__popcll(mask);
            }
        }
    }
    if (!EMIT && lane == 0) counts[blockIdx.x] = n_starts;
}

// length[r] = the distance to the next start (pos holds the low 32 bits of the flattened positions: a run is shorter
// than 2^31 cells, so the difference is exact)
__global__ __launch_bounds__(kFlatThreads) void k_runs_lengths(int64_t n_runs, const uint32_t *__restrict__ pos, uint32_t total_lo,
                                                               int32_t *__restrict__ lengths)
{
    const int64_t r = (int64_t)blockIdx.x * kFlatThreads + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t next = r + 1 < n_runs ? pos[r + 1] : total_lo;
    lengths[r] = (int32_t)(next - pos[r]);
}

}  // namespace

// (the segment table and the scan's arrays: encode_common.h)
struct bsig_runs : SegTable {
    std::unique_ptr<DevPool> res;        // values, lengths and positions of the last encode, at their exact size
    int64_t n_runs = -1;                 // of the last encode (-1: none yet)
    int32_t *values = nullptr, *lengths = nullptr;
};

extern "C" {

int bsig_runs_create(bsig_ctx *ctx, int64_t n_seg, const int64_t *base, const int32_t *len, int32_t stride, bsig_runs **out)
{
    if (!ctx || !out) return fail(BSIG_ERR_ARG, "NULL argument");
    *out = nullptr;
    std::unique_ptr<bsig_runs> R(new bsig_runs);
    if (const int rc = R->build(ctx, n_seg, base, len, stride, "BAMSIGNALS_RUNS_CHUNK_CELLS")) return rc;
    *out = R.release();
    return BSIG_OK;
}

int64_t bsig_runs_n_seg(const bsig_runs *R) { return R ? R->n_seg : 0; }

int64_t bsig_runs_cells(const bsig_runs *R) { return R ? R->total : 0; }

int bsig_runs_encode(bsig_runs *R, const int32_t *src_dev, int64_t *n_runs)
{
    if (!R) return fail(BSIG_ERR_ARG, "runs is NULL");
    if (R->total > 0 && !src_dev) return fail(BSIG_ERR_ARG, "source buffer is NULL");
    HIP_TRY(hipSetDevice(R->ctx->device));
    hipStream_t st = R->ctx->stream;
    R->n_runs = -1;
    R->values = R->lengths = nullptr;
    R->res.reset();
    int64_t total_runs = 0;
    uint32_t *pos = nullptr;
    if (R->total > 0) {
        hipLaunchKernelGGL(k_runs_walk<false>, dim3((unsigned)R->n_st), dim3(kWave), 0, st, src_dev, R->cell0, R->base, R->n_seg,
                           R->stride, R->total, R->chunk, R->counts, nullptr, nullptr, nullptr, nullptr);
        hipLaunchKernelGGL(k_runs_scan, dim3(1), dim3(kScanThreads), 0, st, R->n_st, R->counts, R->st_base, R->d_total);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&total_runs, R->d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (total_runs < 1 || total_runs > R->total) return fail(BSIG_ERR_DEVICE, "run count %lld out of range", (long long)total_runs);
        // the worst case is one run per cell: sized by the count, never blind
        R->res.reset(new DevPool);
        HIP_TRY(R->res->alloc(&R->values, (size_t)total_runs));
        HIP_TRY(R->res->alloc(&R->lengths, (size_t)total_runs));
        HIP_TRY(R->res->alloc(&pos, (size_t)total_runs));
        hipLaunchKernelGGL(k_runs_walk<true>, dim3((unsigned)R->n_st), dim3(kWave), 0, st, src_dev, R->cell0, R->base, R->n_seg,
                           R->stride, R->total, R->chunk, nullptr, R->st_base, R->values, pos, R->seg_off);
        hipLaunchKernelGGL(k_runs_lengths, dim3((unsigned)((total_runs + kFlatThreads - 1) / kFlatThreads)), dim3(kFlatThreads), 0, st,
                           total_runs, pos, (uint32_t)R->total, R->lengths);
    }
    if (R->has_empty || R->total == 0) {
        hipLaunchKernelGGL(k_runs_fill_empty, dim3((unsigned)((R->n_seg + 1 + kFlatThreads - 1) / kFlatThreads)), dim3(kFlatThreads), 0,
                           st, R->n_seg, R->cell0, R->total, total_runs, R->seg_off);
    } else {
        HIP_TRY(hipMemcpyAsync(R->seg_off + R->n_seg, R->d_total, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    R->n_runs = total_runs;
    if (n_runs) *n_runs = total_runs;
    return BSIG_OK;
}

int bsig_runs_device(const bsig_runs *R, int64_t *n_runs, const int64_t **seg_off, const int32_t **values, const int32_t **lengths)
{
    if (!R) return fail(BSIG_ERR_ARG, "runs is NULL");
    if (R->n_runs < 0) return fail(BSIG_ERR_ARG, "nothing has been encoded yet");
    if (n_runs) *n_runs = R->n_runs;
    if (seg_off) *seg_off = R->seg_off;
    if (values) *values = R->values;
    if (lengths) *lengths = R->lengths;
    return BSIG_OK;
}

int bsig_runs_fetch(bsig_runs *R, int64_t *seg_off, int32_t *values, int32_t *lengths)
{
    if (!R) return fail(BSIG_ERR_ARG, "runs is NULL");
    if (R->n_runs < 0) return fail(BSIG_ERR_ARG, "nothing has been encoded yet");
    if (!seg_off || (R->n_runs > 0 && (!values || !lengths))) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    HIP_TRY(hipSetDevice(R->ctx->device));
    int rc = bsig::download_to_host(R->ctx, R->seg_off, seg_off, ((size_t)R->n_seg + 1) * sizeof(int64_t));
    if (rc == BSIG_OK && R->n_runs) rc = bsig::download_to_host(R->ctx, R->values, values, (size_t)R->n_runs * sizeof(int32_t));
    if (rc == BSIG_OK && R->n_runs) rc = bsig::download_to_host(R->ctx, R->lengths, lengths, (size_t)R->n_runs * sizeof(int32_t));
    return rc;
}

void bsig_runs_free(bsig_runs *R)
{
    if (!R) return;
    (void)hipSetDevice(R->ctx->device);
    delete R;
}

}  // extern "C"
