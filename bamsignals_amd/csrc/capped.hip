// Capped coverage, stage 2 (bsig_plan_create_capped with frag_len > 0): from the capped per-base 5' ends to the coverage of
// reads resized to frag_len bases.
//
// Stage 1 (kernels.hip: k_capped_tiles, bins of one base, strands kept) has written, for every range, the capped 5' ends
// of the range widened by frag_len - 1 bases on both sides into a row of the plan's scratch: (forward, reverse) pairs of
// int32 in GENOME order (the widened ranges are all walked as '+' ranges), `lead` pairs in front of the range's first base.
//   k_capped_scan   inclusive prefix sums of a row in place, both strands at once: a wave scan across the lanes, the
//                   waves' totals through LDS, a carry from one round of 256 pairs to the next (as k_sum_scan carries)
//   k_capped_cover  every kept read covers frag_len bases from its 5' end in its own direction, so with PF / PR the prefix
//                   sums of the forward / reverse ends and j = u + lead the pair of the range's base u:
//                       cov[u] = PF[j] - PF[j - L] + PR[j + L - 1] - PR[j - 1]          (planmath.h: capped_window)
//                   a pair below 0 reads as 0, and a base below base 0 (j < 0) is covered by nothing.  A '-' range is
//                   mirrored (cell x is base w - 1 - x) and its strands swap.
//                   The cell goes to bin x / binsize of its range: stored with bins of one base (two rows: one 8-byte
//                   store), otherwise added with an int32 global atomic into the result, which the call has zeroed.
// The prefix sums are unsigned and 32 bits wide: they may wrap, the differences are exact modulo 2^32, and the true value is
// at most the uncapped coverage, whose int32 contract is bamCoverage's.  Both kernels are linear in the scratch whatever
// frag_len is.  One workgroup per range: cutting long ranges into blocks is not done here.
#include <hip/hip_runtime.h>

#include "bsig_types.h"
#include "kernels.h"

namespace {
constexpr int kWave = 64;
constexpr int kCapThreads = 256;

__global__ __launch_bounds__(kCapThreads) void k_capped_scan(const BsigCappedRange *__restrict__ ranges, uint32_t *__restrict__ scratch)
{
    __shared__ uint2 wtot[kCapThreads / kWave];
    const BsigCappedRange r = ranges[blockIdx.x];
    uint2 *row = reinterpret_cast<uint2 *>(scratch + r.s_off);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    uint2 carry = make_uint2(0u, 0u);
    for (int base = 0; base < r.slen; base += kCapThreads) {           // (uniform)
        const int i = base + tid;
        uint2 v = i < r.slen ? row[i] : make_uint2(0u, 0u);
#pragma unroll
        for (int d = 1; d < kWave; d *= 2) {
            const uint32_t ox = __shfl_up(v.x, d), oy = __shfl_up(v.y, d);
            if (lane >= d) { v.x += ox; v.y += oy; }
        }
        if (lane == kWave - 1) wtot[wv] = v;
        __syncthreads();
        uint2 pre = carry, all = make_uint2(0u, 0u);
        for (int k = 0; k < kCapThreads / kWave; ++k) {
            const uint2 s = wtot[k];
            if (k < wv) { pre.x += s.x; pre.y += s.y; }
            all.x += s.x; all.y += s.y;
        }
        __syncthreads();
        if (i < r.slen) row[i] = make_uint2(v.x + pre.x, v.y + pre.y);
        carry.x += all.x; carry.y += all.y;
    }
}

template <bool BINNED>
__global__ __launch_bounds__(kCapThreads) void k_capped_cover(const BsigCappedRange *__restrict__ ranges, const uint32_t *__restrict__ scratch,
                                                              int32_t *__restrict__ out, const int frag_len, const int ss,
                                                              const uint32_t bin_magic, const int bin_shift)
{
    const BsigCappedRange r = ranges[blockIdx.x];
    const uint2 *row = reinterpret_cast<const uint2 *>(scratch + r.s_off);
    // (a pair below 0 is 0; none lies behind the row: clamped all the same, so that no address depends on the arithmetic)
    const auto ps = [&](long long j) {
        if (j < 0) return make_uint2(0u, 0u);
        return row[j < r.slen ? j : r.slen - 1];
    };
    int32_t *dst = out + r.r_off;
    for (int x = threadIdx.x; x < r.w; x += kCapThreads) {
        const int u = r.neg ? r.w - 1 - x : x;
        const long long j = (long long)u + r.lead;
        // (j < 0: a base below base 0, which no read covers; an empty row: nothing at or above base 0)
        const bool none = j < 0 || r.slen <= 0;
        const uint32_t fwd = none ? 0u : ps(j).x - ps(j - frag_len).x;
        const uint32_t rev = none ? 0u : ps(j + frag_len - 1).y - ps(j - 1).y;
        const uint32_t sense = r.neg ? rev : fwd, anti = r.neg ? fwd : rev;
        if constexpr (!BINNED) {
            if (ss) *reinterpret_cast<int2 *>(dst + 2 * (size_t)x) = make_int2((int)sense, (int)anti);
            else dst[x] = (int)(sense + anti);
        } else {
            const size_t b = __umulhi((uint32_t)x, bin_magic) >> bin_shift;
            if (ss) {
                if (sense) atomicAdd(dst + 2 * b, (int)sense);
                if (anti) atomicAdd(dst + 2 * b + 1, (int)anti);
            } else if (sense + anti) {
                atomicAdd(dst + b, (int)(sense + anti));
            }
        }
    }
}
}  // namespace

namespace bsig {
hipError_t launch_capped_scan(const BsigCappedRange *ranges, int64_t n_ranges, uint32_t *scratch, hipStream_t st)
{
    if (n_ranges <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_capped_scan, dim3((unsigned)n_ranges), dim3(kCapThreads), 0, st, ranges, scratch);
    return hipGetLastError();
}

hipError_t launch_capped_cover(const BsigCappedRange *ranges, int64_t n_ranges, const uint32_t *scratch, int frag_len, int ss,
                               bool binned, uint32_t bin_magic, int bin_shift, int32_t *out, hipStream_t st)
{
    if (n_ranges <= 0) return hipSuccess;
    if (frag_len < 1) return hipErrorInvalidValue;
    if (binned)
        hipLaunchKernelGGL(k_capped_cover<true>, dim3((unsigned)n_ranges), dim3(kCapThreads), 0, st, ranges, scratch, out, frag_len, ss,
                           bin_magic, bin_shift);
    else
        hipLaunchKernelGGL(k_capped_cover<false>, dim3((unsigned)n_ranges), dim3(kCapThreads), 0, st, ranges, scratch, out, frag_len, ss,
                           bin_magic, bin_shift);
    return hipGetLastError();
}
}  // namespace bsig
