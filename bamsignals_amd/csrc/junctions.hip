// Splice junctions: the gaps of a spliced set as a resident table, and the reads that support each junction of a range.
//
// A JUNCTION ROW is one gap of one read (splice_walk.h says what a gap is): its reference, the gap's first and last base, the
// read's flag and mapq, and its ANCHOR = min(left, right) -- the reference bases of the aligned blocks that touch the gap on
// either side (the stretch back to the read's previous gap or its pos, forward to its next gap or its end; 0 where the gap
// opens or closes the read).  Both follow from the gap table's neighbouring rows and the pos / end columns.
//
// The table (junctions_build, called by spliced_layout while the gap table and the read columns stand on the device):
//   k_junc_emit     one thread per gap row: two sort keys (end; reference << 32 | start, both biased so that -1 sorts first),
//                   flag | mapq << 16 and the anchor
//   sort            two stable rocPRIM radix sorts, by end and then by (reference, start): ties keep the earlier order, so the
//                   rows stand by (reference, start, end) and equal junctions are neighbours
//   k_junc_gather   the four resident columns and the per-reference row offsets jref_off[n_ref + 1]
//
// The query (junctions_query): launches with a boundary between every two of them -- no workgroup ever waits for another one:
//   k_junc_slices   one thread per range: the rows [a, b) of its reference with loc <= start <= loc + len - 1 (two binary
//                   searches in the start column)
//   scan            64-bit work offsets of the slice lengths (launch_gap_scan); the host reads their total
//   k_junc_mark     one work item per (range, row of its slice): the item's range by a binary search in the work offsets; the
//                   item is a HEAD iff it is its slice's first or (start, end) differs from the row before -- decided on the
//                   unfiltered rows.  Heads per workgroup, their scan in a launch of its own: an item's SEGMENT is the number
//                   of heads up to and including it, less one.  The host reads the number of segments
//   k_junc_count    per item keep = end inside the range, the flag / mapq filter, the anchor rule.  The lanes of a wave that
//                   share a segment stand side by side (segments never decrease along the items): a segmented scan across the
//                   lanes sums the kept sense and antisense rows and takes the largest kept anchor, the run's last lane commits
//                   with integer atomics into the zeroed cells of the segment -- at most one commit per (segment, wave), and
//                   integer adds and a max commute: the result is the same on every run.  The head stores start, end, range
//   k_junc_keep     segments with a kept row, counted per workgroup; scanned; the host reads their number
//   k_junc_compact  the kept segments in order -- the caller's range order, ascending by (start, end) inside a range -- and one
//                   integer add per kept segment to its range's count; the scan of those counts is seg_off
// Only the compacted columns are downloaded.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "junctions.h"
#include "splice.h"

using bsig::fail;
using bsig::GapRow;
using bsig::GapTable;

namespace {

constexpr int kJuncThreads = 256;       // rows, items or segments per workgroup
constexpr int kWaveLanes = 64;
constexpr int64_t kMaxItems = ((int64_t)1 << 32) - 8;

inline unsigned groups_of(int64_t n) { return (unsigned)((n + kJuncThreads - 1) / kJuncThreads); }

// the reference of read i: the largest r < n_ref with ref_off[r] <= i (as splice.hip's k_block_emit finds it)
__device__ __forceinline__ int32_t ref_of(const int64_t *__restrict__ ref_off, int32_t n_ref, int64_t i)
{
    int32_t lo = 0, hi = n_ref - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (ref_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJuncThreads) void k_junc_emit(int64_t n_rows, const GapRow *__restrict__ rows, int32_t n_ref,
                                                            const int64_t *__restrict__ ref_off, const int32_t *__restrict__ pos,
                                                            const int32_t *__restrict__ end, const uint16_t *__restrict__ flag,
                                                            const uint8_t *__restrict__ mapq, uint32_t *__restrict__ key_end,
                                                            uint64_t *__restrict__ key_ref_start, uint32_t *__restrict__ row_id,
                                                            uint32_t *__restrict__ fm, int32_t *__restrict__ anchor)
{
    const int64_t g = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    if (g >= n_rows) return;
    const GapRow r = rows[g];
    const int64_t i = r.read;
    // the aligned bases on either side: back to the read's previous gap or its pos, forward to its next gap or its end
    int64_t left = g > 0 && rows[g - 1].read == i ? (int64_t)r.start - rows[g - 1].end - 1 : (int64_t)r.start - pos[i];
    int64_t right = g + 1 < n_rows && rows[g + 1].read == i ? (int64_t)rows[g + 1].start - r.end - 1 : (int64_t)end[i] - r.end;
    left = left < 0 ? 0 : left;
    right = right < 0 ? 0 : right;
    const int64_t a = left < right ? left : right;
    key_end[g] = (uint32_t)r.end ^ 0x80000000u;           // signed order: -1 sorts before 0
    key_ref_start[g] = ((uint64_t)(uint32_t)ref_of(ref_off, n_ref, i) << 32) | ((uint32_t)r.start ^ 0x80000000u);
    row_id[g] = (uint32_t)g;
    fm[g] = (uint32_t)flag[i] | ((uint32_t)mapq[i] << 16);
    anchor[g] = a > 0x7FFFFFFF ? 0x7FFFFFFF : (int32_t)a;
}

// the second sort's keys in the first sort's order
__global__ __launch_bounds__(kJuncThreads) void k_junc_rekey(int64_t n_rows, const uint32_t *__restrict__ order,
                                                             const uint64_t *__restrict__ key, uint64_t *__restrict__ key_out)
{
    const int64_t k = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    if (k < n_rows) key_out[k] = key[order[k]];
}

// the resident columns of the sorted rows; jref_off[r] = the first row of reference r or of a later one (written by the row
// that opens a reference for every reference since the row before; the last row closes the table)
__global__ __launch_bounds__(kJuncThreads) void k_junc_gather(int64_t n_rows, const uint32_t *__restrict__ order,
                                                              const uint64_t *__restrict__ key_sorted, const GapRow *__restrict__ rows,
                                                              const uint32_t *__restrict__ fm, const int32_t *__restrict__ anchor,
                                                              int32_t n_ref, int32_t *__restrict__ o_start, int32_t *__restrict__ o_end,
                                                              uint32_t *__restrict__ o_fm, int32_t *__restrict__ o_anchor,
                                                              int64_t *__restrict__ jref_off)
{
    const int64_t k = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    if (k >= n_rows) return;
    const uint32_t j = order[k];
    o_start[k] = rows[j].start;
    o_end[k] = rows[j].end;
    o_fm[k] = fm[j];
    o_anchor[k] = anchor[j];
    int64_t ref = (int64_t)(key_sorted[k] >> 32);
    ref = ref < n_ref ? ref : n_ref - 1;
    const int64_t before = k > 0 ? (int64_t)(key_sorted[k - 1] >> 32) : -1;
    for (int64_t r = before + 1; r <= ref; ++r) jref_off[r] = k;
    if (k == n_rows - 1)
        for (int64_t r = ref + 1; r <= n_ref; ++r) jref_off[r] = n_rows;
}

// ---- the query -----------------------------------------------------------------------------------------------------------
struct JuncFilter {
    int32_t mapqual;
    uint32_t requiredF, filteredF;
    int32_t min_anchor;
    int32_t ss;
};

// a row's flag / mapq filter: the rule of every other call (kernels.hip: fm_rejected)
__device__ __forceinline__ bool junc_rejected(const JuncFilter &F, uint32_t fm)
{
    const uint32_t nf = ~(fm & 0xFFFFu);
    const int mapq = (int)((fm >> 16) & 0xFFu);
    return (mapq < F.mapqual) | ((F.requiredF & nf) != 0u) | ((F.filteredF & nf) == 0u);
}

// the first k in [lo, hi) with col[k] >= v (above == false) or col[k] > v (above == true)
__device__ __forceinline__ int64_t first_row(const int32_t *__restrict__ col, int64_t lo, int64_t hi, int64_t v, bool above)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t c = col[mid];
        if (above ? c <= v : c < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kJuncThreads) void k_junc_slices(int64_t n, int32_t n_ref, const int32_t *__restrict__ rid,
                                                              const int32_t *__restrict__ loc, const int32_t *__restrict__ len,
                                                              const int64_t *__restrict__ jref_off, const int32_t *__restrict__ jstart,
                                                              uint32_t *__restrict__ slice_a, uint32_t *__restrict__ slice_n)
{
    const int64_t i = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t r = rid[i], w = len[i];
    uint32_t a = 0, c = 0;
    if (w > 0 && r >= 0 && r < n_ref) {
        const int64_t r0 = jref_off[r], r1 = jref_off[r + 1];
        const int64_t lo = loc[i], hi = lo + w - 1;
        const int64_t ka = first_row(jstart, r0, r1, lo, false);
        const int64_t kb = first_row(jstart, ka, r1, hi, true);
        a = (uint32_t)ka;
        c = (uint32_t)(kb - ka);
    }
    slice_a[i] = a;
    slice_n[i] = c;
}

// the range of work item w: the largest i with work_off[i] <= w (ranges without rows share their offset with the next range
// that has some: the largest is the one that holds the item)
__device__ __forceinline__ int64_t range_of(const int64_t *__restrict__ work_off, int64_t n, int64_t w)
{
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (work_off[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kJuncThreads) void k_junc_mark(int64_t n_items, int64_t n, const int64_t *__restrict__ work_off,
                                                            const uint32_t *__restrict__ slice_a, const int32_t *__restrict__ jstart,
                                                            const int32_t *__restrict__ jend, uint32_t *__restrict__ item_range,
                                                            uint32_t *__restrict__ item_row, uint8_t *__restrict__ item_head,
                                                            uint32_t *__restrict__ group_heads)
{
    __shared__ uint32_t scratch[kJuncThreads];
    const int64_t w = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    uint32_t head = 0;
    if (w < n_items) {
        const int64_t i = range_of(work_off, n, w);
        const int64_t first = work_off[i];
        const int64_t row = (int64_t)slice_a[i] + (w - first);
        head = w == first || jstart[row] != jstart[row - 1] || jend[row] != jend[row - 1];
        item_range[w] = (uint32_t)i;
        item_row[w] = (uint32_t)row;
        item_head[w] = (uint8_t)head;
    }
    uint32_t total;
    bsig::block_exclusive_scan<kJuncThreads>(head, scratch, &total);
    if (threadIdx.x == 0) group_heads[blockIdx.x] = total;
}

__global__ __launch_bounds__(kJuncThreads) void k_junc_count(int64_t n_items, const uint32_t *__restrict__ item_range,
                                                             const uint32_t *__restrict__ item_row, const uint8_t *__restrict__ item_head,
                                                             const int64_t *__restrict__ group_base, const int32_t *__restrict__ loc,
                                                             const int32_t *__restrict__ len, const int32_t *__restrict__ strand,
                                                             const int32_t *__restrict__ jstart, const int32_t *__restrict__ jend,
                                                             const uint32_t *__restrict__ jfm, const int32_t *__restrict__ janchor,
                                                             JuncFilter F, int64_t n_seg, int32_t *__restrict__ seg_start,
                                                             int32_t *__restrict__ seg_end, uint32_t *__restrict__ seg_range,
                                                             uint32_t *__restrict__ seg_sense, uint32_t *__restrict__ seg_anti,
                                                             uint32_t *__restrict__ seg_max)
{
    __shared__ uint32_t scratch[kJuncThreads];
    const int64_t w = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    const bool valid = w < n_items;
    const uint32_t head = valid ? item_head[w] : 0u;
    uint32_t total;
    const uint32_t before = bsig::block_exclusive_scan<kJuncThreads>(head, scratch, &total);
    // heads up to and including this item, less one (an item that is no head belongs to the segment of the head before it,
    // which may stand in an earlier workgroup); no item: a segment no item has
    const int64_t seg = valid ? group_base[blockIdx.x] + before + head - 1 : -1;
    uint32_t sense = 0, anti = 0, best = 0;
    if (valid) {
        const uint32_t i = item_range[w], row = item_row[w];
        const int64_t hi = (int64_t)loc[i] + len[i] - 1;
        const uint32_t fm = jfm[row];
        const int32_t anchor = janchor[row];
        const bool keep = (int64_t)jend[row] <= hi && !junc_rejected(F, fm) && anchor >= F.min_anchor;
        // sense: the row's 0x10 bit agrees with the range's strand, '*' counted as '+' (as bamCount splits)
        const bool is_anti = F.ss && (((fm & 0x10u) != 0u) != (strand[i] < 0));
        sense = keep && !is_anti;
        anti = keep && is_anti;
        best = keep ? (uint32_t)anchor : 0u;
        if (head && seg >= 0 && seg < n_seg) {
            seg_start[seg] = jstart[row];
            seg_end[seg] = jend[row];
            seg_range[seg] = i;
        }
    }
    // inclusive segmented scan across the lanes of the wave: a lane takes from the lane d below it iff that lane is in its
    // segment (segments never decrease, so every lane between them is too)
    const int lane = threadIdx.x & (kWaveLanes - 1);
#pragma unroll
    for (int d = 1; d < kWaveLanes; d <<= 1) {
        const int64_t seg_up = __shfl_up(seg, d);
        const uint32_t s_up = __shfl_up(sense, d), a_up = __shfl_up(anti, d), b_up = __shfl_up(best, d);
        if (lane >= d && seg_up == seg) {
            sense += s_up;
            anti += a_up;
            best = b_up > best ? b_up : best;
        }
    }
    // the last lane of every run of equal segments commits: at most one commit per (segment, wave)
    const int64_t seg_next = __shfl_down(seg, 1);
    const bool last = lane == kWaveLanes - 1 || seg_next != seg;
    if (valid && last && seg >= 0 && seg < n_seg && (sense | anti)) {
        if (sense) atomicAdd(&seg_sense[seg], sense);
        if (anti) atomicAdd(&seg_anti[seg], anti);
        atomicMax(&seg_max[seg], best);
    }
}

__global__ __launch_bounds__(kJuncThreads) void k_junc_keep(int64_t n_seg, const uint32_t *__restrict__ seg_sense,
                                                            const uint32_t *__restrict__ seg_anti, uint32_t *__restrict__ group_kept)
{
    __shared__ uint32_t scratch[kJuncThreads];
    const int64_t s = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    const uint32_t kept = s < n_seg && (seg_sense[s] | seg_anti[s]) != 0u;
    uint32_t total;
    bsig::block_exclusive_scan<kJuncThreads>(kept, scratch, &total);
    if (threadIdx.x == 0) group_kept[blockIdx.x] = total;
}

__global__ __launch_bounds__(kJuncThreads) void k_junc_compact(int64_t n_seg, int64_t n_kept, int64_t n, int32_t ss,
                                                               const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_end,
                                                               const uint32_t *__restrict__ seg_range, const uint32_t *__restrict__ seg_sense,
                                                               const uint32_t *__restrict__ seg_anti, const uint32_t *__restrict__ seg_max,
                                                               const int64_t *__restrict__ group_base, int32_t *__restrict__ o_start,
                                                               int32_t *__restrict__ o_end, uint32_t *__restrict__ o_count,
                                                               int32_t *__restrict__ o_max, uint32_t *__restrict__ range_kept)
{
    __shared__ uint32_t scratch[kJuncThreads];
    const int64_t s = (int64_t)blockIdx.x * kJuncThreads + threadIdx.x;
    const uint32_t kept = s < n_seg && (seg_sense[s] | seg_anti[s]) != 0u;
    uint32_t total;
    const uint32_t before = bsig::block_exclusive_scan<kJuncThreads>(kept, scratch, &total);
    if (!kept) return;
    const int64_t at = group_base[blockIdx.x] + before;
    const uint32_t i = seg_range[s];
    if (at >= n_kept || (int64_t)i >= n) return;        // (never out of bounds)
    o_start[at] = seg_start[s];
    o_end[at] = seg_end[s];
    if (ss) {
        o_count[2 * at] = seg_sense[s];
        o_count[2 * at + 1] = seg_anti[s];
    } else {
        o_count[at] = seg_sense[s];
    }
    o_max[at] = (int32_t)seg_max[s];
    atomicAdd(&range_kept[i], 1u);
}

// per-workgroup counts -> their 64-bit bases on the device and their total on the host
int scan_groups(hipStream_t st, int64_t n_groups, const uint32_t *d_counts, int64_t *d_base, int64_t *d_total, int64_t *total)
{
    HIP_TRY(bsig::launch_gap_scan(n_groups, d_counts, d_base, d_total, st));
    HIP_TRY(hipMemcpyAsync(total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BSIG_OK;
}

}  // namespace

namespace bsig {

int junctions_rule(int32_t min_anchor)
{
    if (min_anchor < 0) return fail(BSIG_ERR_ARG, "min_anchor must not be negative (%d given)", (int)min_anchor);
    return BSIG_OK;
}

int junctions_build(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int64_t *d_ref_off, const int32_t *d_pos,
                    const int32_t *d_end, const uint16_t *d_flag, const uint8_t *d_mapq, const GapTable &gaps)
{
    hipStream_t st = ctx->stream;
    bsig_reads::Junctions &J = R->junc;
    J = bsig_reads::Junctions{};
    J.h_ref_off.assign((size_t)std::max(n_ref, 0) + 1, 0);
    const int64_t g = gaps.n;
    if (g >= kMaxItems) return fail(BSIG_ERR_ARG, "more than 2^32 - 8 gap rows in a spliced set");
    if (n <= 0 || n_ref <= 0 || g <= 0) return BSIG_OK;
    DevPool tmp(2.0);
    const size_t cap = (size_t)g;
    uint32_t *d_key_end, *d_key_end_sorted, *d_row, *d_order1, *d_order, *d_fm;
    uint64_t *d_key, *d_key1, *d_key_sorted;
    int32_t *d_anchor;
    HIP_TRY(tmp.alloc(&d_key_end, cap));
    HIP_TRY(tmp.alloc(&d_key_end_sorted, cap));
    HIP_TRY(tmp.alloc(&d_row, cap));
    HIP_TRY(tmp.alloc(&d_order1, cap));
    HIP_TRY(tmp.alloc(&d_order, cap));
    HIP_TRY(tmp.alloc(&d_fm, cap));
    HIP_TRY(tmp.alloc(&d_key, cap));
    HIP_TRY(tmp.alloc(&d_key1, cap));
    HIP_TRY(tmp.alloc(&d_key_sorted, cap));
    HIP_TRY(tmp.alloc(&d_anchor, cap));
    hipLaunchKernelGGL(k_junc_emit, dim3(groups_of(g)), dim3(kJuncThreads), 0, st, g, gaps.rows, n_ref, d_ref_off, d_pos, d_end, d_flag,
                       d_mapq, d_key_end, d_key, d_row, d_fm, d_anchor);
    HIP_TRY(hipGetLastError());
    // stable sorts: by end, then by (reference, start)
    unsigned ref_bits = 1;
    while (ref_bits < 31 && ((int64_t)1 << ref_bits) < n_ref) ++ref_bits;
    size_t bytes1 = 0, bytes2 = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes1, d_key_end, d_key_end_sorted, d_row, d_order1, cap, 0u, 32u, st));
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes2, d_key1, d_key_sorted, d_order1, d_order, cap, 0u, 32u + ref_bits, st));
    uint8_t *d_sort_tmp;
    HIP_TRY(tmp.alloc(&d_sort_tmp, std::max<size_t>(std::max(bytes1, bytes2), 1)));
    HIP_TRY(rocprim::radix_sort_pairs(d_sort_tmp, bytes1, d_key_end, d_key_end_sorted, d_row, d_order1, cap, 0u, 32u, st));
    hipLaunchKernelGGL(k_junc_rekey, dim3(groups_of(g)), dim3(kJuncThreads), 0, st, g, d_order1, d_key, d_key1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs(d_sort_tmp, bytes2, d_key1, d_key_sorted, d_order1, d_order, cap, 0u, 32u + ref_bits, st));
    // the resident columns: the set's own pool, so that hbm_bytes and the cache's budget count them
    int32_t *o_start, *o_end, *o_anchor;
    uint32_t *o_fm;
    int64_t *o_ref_off;
    HIP_TRY(R->pool.alloc(&o_start, cap));
    HIP_TRY(R->pool.alloc(&o_end, cap));
    HIP_TRY(R->pool.alloc(&o_fm, cap));
    HIP_TRY(R->pool.alloc(&o_anchor, cap));
    HIP_TRY(R->pool.alloc(&o_ref_off, (size_t)n_ref + 1));
    hipLaunchKernelGGL(k_junc_gather, dim3(groups_of(g)), dim3(kJuncThreads), 0, st, g, d_order, d_key_sorted, gaps.rows, d_fm, d_anchor,
                       n_ref, o_start, o_end, o_fm, o_anchor, o_ref_off);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(J.h_ref_off.data(), o_ref_off, ((size_t)n_ref + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));          // (tmp goes away)
    J.n = g;
    J.start = o_start; J.end = o_end; J.fm = o_fm; J.anchor = o_anchor; J.ref_off = o_ref_off;
    return BSIG_OK;
}

int junctions_query(const bsig_reads *R, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                    int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_anchor, int32_t ss, EncodedColumns *out)
{
    if (!R || !out) return fail(BSIG_ERR_ARG, "NULL argument");
    if (const int rc = junctions_rule(min_anchor)) return rc;
    if (!R->spliced) return fail(BSIG_ERR_ARG, "junctions need spliced reads: a plain set keeps no gap table");
    if (n < 0 || (n > 0 && (!rid || !loc || !len || !strand))) return fail(BSIG_ERR_ARG, "range arrays missing");
    if (n >= kMaxItems) return fail(BSIG_ERR_ARG, "more than 2^32 - 8 ranges in a junction query");
    for (int64_t i = 0; i < n; ++i) {
        if (len[i] < 0) return fail(BSIG_ERR_ARG, "range %lld has a negative width", (long long)i);
        if (rid[i] < 0 || rid[i] >= R->n_ref) return fail(BSIG_ERR_ARG, "range %lld: reference %d is not one of the set's %d", (long long)i, (int)rid[i], (int)R->n_ref);
    }
    const bool stranded = ss != 0;
    out->n_seg = n;
    out->seg_off.assign((size_t)n + 1, 0);
    for (int c = 0; c < EncodedColumns::kMaxCols; ++c) out->col[c].clear();
    const bsig_reads::Junctions &J = R->junc;
    if (n == 0 || J.n == 0) return BSIG_OK;
    bsig_ctx *ctx = R->ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    DevPool tmp(2.0);
    // ---- the ranges, their slices, the work offsets ------------------------------------------------------------------
    int32_t *d_rid, *d_loc, *d_len, *d_strand;
    uint32_t *d_slice_a, *d_slice_n;
    int64_t *d_work_off, *d_total;
    HIP_TRY(tmp.alloc(&d_rid, (size_t)n));
    HIP_TRY(tmp.alloc(&d_loc, (size_t)n));
    HIP_TRY(tmp.alloc(&d_len, (size_t)n));
    HIP_TRY(tmp.alloc(&d_strand, (size_t)n));
    HIP_TRY(tmp.alloc(&d_slice_a, (size_t)n));
    HIP_TRY(tmp.alloc(&d_slice_n, (size_t)n));
    HIP_TRY(tmp.alloc(&d_work_off, (size_t)n + 1));
    HIP_TRY(tmp.alloc(&d_total, 1));
    HIP_TRY(hipMemcpyAsync(d_rid, rid, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_loc, loc, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_len, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_strand, strand, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_junc_slices, dim3(groups_of(n)), dim3(kJuncThreads), 0, st, n, R->n_ref, d_rid, d_loc, d_len, J.ref_off, J.start,
                       d_slice_a, d_slice_n);
    HIP_TRY(hipGetLastError());
    int64_t n_items = 0;
    if (const int rc = scan_groups(st, n, d_slice_n, d_work_off, d_total, &n_items)) return rc;
    if (n_items >= kMaxItems)
        return fail(BSIG_ERR_ARG, "a junction query of more than 2^32 - 8 (range, row) pairs (%lld): ask for fewer ranges at a time", (long long)n_items);
    if (n_items <= 0) return BSIG_OK;
    // ---- heads, segments ---------------------------------------------------------------------------------------------
    const int64_t item_groups = groups_of(n_items);
    uint32_t *d_item_range, *d_item_row, *d_group_heads;
    uint8_t *d_item_head;
    int64_t *d_group_base;
    HIP_TRY(tmp.alloc(&d_item_range, (size_t)n_items));
    HIP_TRY(tmp.alloc(&d_item_row, (size_t)n_items));
    HIP_TRY(tmp.alloc(&d_item_head, (size_t)n_items));
    HIP_TRY(tmp.alloc(&d_group_heads, (size_t)item_groups));
    HIP_TRY(tmp.alloc(&d_group_base, (size_t)item_groups));
    hipLaunchKernelGGL(k_junc_mark, dim3((unsigned)item_groups), dim3(kJuncThreads), 0, st, n_items, n, d_work_off, d_slice_a, J.start, J.end,
                       d_item_range, d_item_row, d_item_head, d_group_heads);
    HIP_TRY(hipGetLastError());
    int64_t n_seg = 0;
    if (const int rc = scan_groups(st, item_groups, d_group_heads, d_group_base, d_total, &n_seg)) return rc;
    if (n_seg <= 0 || n_seg > n_items) return fail(BSIG_ERR_DEVICE, "junction segment count %lld out of range", (long long)n_seg);
    // ---- counts per segment ------------------------------------------------------------------------------------------
    const int64_t seg_groups = groups_of(n_seg);
    int32_t *d_seg_start, *d_seg_end;
    uint32_t *d_seg_range, *d_cells, *d_group_kept, *d_range_kept;
    int64_t *d_kept_base;
    HIP_TRY(tmp.alloc(&d_seg_start, (size_t)n_seg));
    HIP_TRY(tmp.alloc(&d_seg_end, (size_t)n_seg));
    HIP_TRY(tmp.alloc(&d_seg_range, (size_t)n_seg));
    HIP_TRY(tmp.alloc(&d_cells, 3 * (size_t)n_seg));        // sense, antisense, largest anchor: one block, one memset
    HIP_TRY(tmp.alloc(&d_group_kept, (size_t)seg_groups));
    HIP_TRY(tmp.alloc(&d_kept_base, (size_t)seg_groups));
    HIP_TRY(tmp.alloc(&d_range_kept, (size_t)n));
    uint32_t *d_sense = d_cells, *d_anti = d_cells + n_seg, *d_max = d_cells + 2 * n_seg;
    HIP_TRY(hipMemsetAsync(d_cells, 0, 3 * (size_t)n_seg * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(d_range_kept, 0, (size_t)n * sizeof(uint32_t), st));
    const JuncFilter F{mapqual, (uint32_t)requiredF, (uint32_t)filteredF, min_anchor, stranded ? 1 : 0};
    hipLaunchKernelGGL(k_junc_count, dim3((unsigned)item_groups), dim3(kJuncThreads), 0, st, n_items, d_item_range, d_item_row, d_item_head,
                       d_group_base, d_loc, d_len, d_strand, J.start, J.end, J.fm, J.anchor, F, n_seg, d_seg_start, d_seg_end, d_seg_range,
                       d_sense, d_anti, d_max);
    hipLaunchKernelGGL(k_junc_keep, dim3((unsigned)seg_groups), dim3(kJuncThreads), 0, st, n_seg, d_sense, d_anti, d_group_kept);
    HIP_TRY(hipGetLastError());
    int64_t n_kept = 0;
    if (const int rc = scan_groups(st, seg_groups, d_group_kept, d_kept_base, d_total, &n_kept)) return rc;
    if (n_kept < 0 || n_kept > n_seg) return fail(BSIG_ERR_DEVICE, "junction count %lld out of range", (long long)n_kept);
    if (n_kept == 0) return BSIG_OK;
    // ---- the kept segments in order, the ranges' offsets ---------------------------------------------------------------
    const size_t per = stranded ? 2 : 1;
    int32_t *d_o_start, *d_o_end, *d_o_max;
    uint32_t *d_o_count;
    int64_t *d_seg_off;
    HIP_TRY(tmp.alloc(&d_o_start, (size_t)n_kept));
    HIP_TRY(tmp.alloc(&d_o_end, (size_t)n_kept));
    HIP_TRY(tmp.alloc(&d_o_count, per * (size_t)n_kept));
    HIP_TRY(tmp.alloc(&d_o_max, (size_t)n_kept));
    HIP_TRY(tmp.alloc(&d_seg_off, (size_t)n + 1));
    hipLaunchKernelGGL(k_junc_compact, dim3((unsigned)seg_groups), dim3(kJuncThreads), 0, st, n_seg, n_kept, n, stranded ? 1 : 0, d_seg_start,
                       d_seg_end, d_seg_range, d_sense, d_anti, d_max, d_kept_base, d_o_start, d_o_end, d_o_count, d_o_max, d_range_kept);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_gap_scan(n, d_range_kept, d_seg_off, d_seg_off + n, st));
    HIP_TRY(hipStreamSynchronize(st));
    // ---- only the compacted columns leave the device -----------------------------------------------------------------
    const size_t elem[4] = {sizeof(int32_t), sizeof(int32_t), per * sizeof(uint32_t), sizeof(int32_t)};
    const void *src[4] = {d_o_start, d_o_end, d_o_count, d_o_max};
    int rc = download_to_host(ctx, d_seg_off, out->seg_off.data(), ((size_t)n + 1) * sizeof(int64_t));
    for (int c = 0; c < 4 && rc == BSIG_OK; ++c) {
        out->col[c].resize((size_t)n_kept * elem[c]);
        rc = download_to_host(ctx, src[c], out->col[c].data(), out->col[c].size());
    }
    if (rc == BSIG_OK && out->seg_off.back() != n_kept) rc = fail(BSIG_ERR_DEVICE, "junction offsets do not add up");
    return rc;
}

}  // namespace bsig

extern "C" {

int64_t bsig_reads_n_junction_rows(const bsig_reads *reads) { return reads ? reads->junc.n : 0; }

int bsig_reads_junctions(const bsig_reads *reads, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len,
                         const int32_t *strand, int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_anchor, int32_t ss,
                         bsig_junctions_result **result)
{
    if (!result) return fail(BSIG_ERR_ARG, "result is NULL");
    *result = nullptr;
    if (!reads) return fail(BSIG_ERR_ARG, "reads is NULL");
    std::unique_ptr<bsig_junctions_result> res(new bsig_junctions_result);
    res->ss = ss != 0;
    const int rc = bsig::junctions_query(reads, n, rid, loc, len, strand, mapqual, requiredF, filteredF, min_anchor, ss, res.get());
    if (rc == BSIG_OK) *result = res.release();
    return rc;
}

int64_t bsig_junctions_result_n_seg(const bsig_junctions_result *r) { return r ? r->n_seg : 0; }

int64_t bsig_junctions_result_n_junctions(const bsig_junctions_result *r) { return r ? r->entries() : 0; }

int bsig_junctions_result_copy(const bsig_junctions_result *r, int64_t *seg_off, int32_t *start, int32_t *end, uint32_t *count,
                               int32_t *max_anchor)
{
    if (!r || !seg_off) return fail(BSIG_ERR_ARG, "NULL argument");
    const size_t n = (size_t)r->entries();
    if (n && (!start || !end || !count || !max_anchor)) return fail(BSIG_ERR_ARG, "output buffer is NULL");
    memcpy(seg_off, r->seg_off.data(), r->seg_off.size() * sizeof(int64_t));
    void *const dst[4] = {start, end, count, max_anchor};
    for (int c = 0; n && c < 4; ++c) memcpy(dst[c], r->col[c].data(), r->col[c].size());
    return BSIG_OK;
}

void bsig_junctions_result_free(bsig_junctions_result *r) { delete r; }

}  // extern "C"
