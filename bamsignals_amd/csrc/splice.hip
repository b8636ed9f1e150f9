// Spliced reads: coverage that skips N gaps, by handing the unchanged kernels other intervals.
//
// A spliced bsig_reads holds one row per aligned BLOCK of a read in place of one row per read (splice_walk.h says what a gap
// and a block are); every row carries its read's flag, mapq and tlen.  It is an ordinary resident set -- span classes, bucket
// indexes, the packed class -- so plans, pileup and reduction kernels, runs and views work on it as they are.  Made here:
//
//   gap table   (read, gap start, gap end) in read order: k_gap_count per read, launch_gap_scan, k_gap_emit -- from the CIGAR
//               columns (this file), or from the inflated stream right behind k_bam_extract (devdecode.hip: same walk);
//   split       k_block_count per read (its gaps found by binary search in the table), the scan, k_block_emit: the block
//               rows in read order with their sort key (reference << 32 | start, biased so that -1 sorts first);
//   order       rocPRIM's device radix sort of (key, row): stable, so ties keep BAM order and then block order;
//   gather      k_block_gather: the five columns of the sorted rows; ref_off' follows from the scan (the rows of one
//               reference stay contiguous), and layout_from_device does the rest.
// The gap table is not thrown away behind the split: junctions.hip keeps it with the set, sorted, as its junction table.
// Nor are the rows in read order: k_block_emit writes them into the set's own pool with every read's slice of them and its
// flag | mapq << 16 -- the READ TABLE (runtime_internal.h), which genecounts.hip walks one read at a time.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include <rocprim/device/device_radix_sort.hpp>

#include "junctions.h"
#include "kernels.h"
#include "splice.h"

using bsig::fail;
using bsig::GapRow;
using bsig::GapTable;

namespace {

constexpr int kSpliceThreads = 256;     // reads (or rows) per workgroup
constexpr int kScanThreads = 1024;

// ---- the gap table from CIGAR columns ----------------------------------------------------------------------------------
// per read its number of gaps, per workgroup their sum
__global__ __launch_bounds__(kSpliceThreads) void k_gap_count(int64_t n, const int32_t *__restrict__ pos, const uint16_t *__restrict__ flag,
                                                              const int64_t *__restrict__ cigar_off, const uint32_t *__restrict__ cigar,
                                                              uint32_t *__restrict__ read_gaps, uint32_t *__restrict__ group_gaps)
{
    __shared__ uint32_t scratch[kSpliceThreads];
    const int64_t i = (int64_t)blockIdx.x * kSpliceThreads + threadIdx.x;
    uint32_t c = 0;
    if (i < n) {
        const int64_t k0 = cigar_off[i], k1 = cigar_off[i + 1];
        c = bsig::walk_gaps(pos[i], flag[i], (uint32_t)(k1 - k0), [&](uint32_t q) { return cigar[k0 + q]; },
                            [](uint32_t, int32_t, int32_t) {});
        read_gaps[i] = c;
    }
    uint32_t total;
    bsig::block_exclusive_scan<kSpliceThreads>(c, scratch, &total);
    if (threadIdx.x == 0) group_gaps[blockIdx.x] = total;
}

// the rows: a read's gaps stand at group_base[workgroup] + the gaps of the workgroup's reads before it
__global__ __launch_bounds__(kSpliceThreads) void k_gap_emit(int64_t n, const int32_t *__restrict__ pos, const uint16_t *__restrict__ flag,
                                                             const int64_t *__restrict__ cigar_off, const uint32_t *__restrict__ cigar,
                                                             const uint32_t *__restrict__ read_gaps, const int64_t *__restrict__ group_base,
                                                             GapRow *__restrict__ rows, int64_t n_rows)
{
    __shared__ uint32_t scratch[kSpliceThreads];
    const int64_t i = (int64_t)blockIdx.x * kSpliceThreads + threadIdx.x;
    const uint32_t c = i < n ? read_gaps[i] : 0u;
    uint32_t total;
    const uint32_t before = bsig::block_exclusive_scan<kSpliceThreads>(c, scratch, &total);
    if (!c) return;
    const int64_t at = group_base[blockIdx.x] + before;
    const int64_t k0 = cigar_off[i], k1 = cigar_off[i + 1];
    bsig::walk_gaps(pos[i], flag[i], (uint32_t)(k1 - k0), [&](uint32_t q) { return cigar[k0 + q]; },
                    [&](uint32_t k, int32_t s, int32_t e) {
                        if (k < c && at + k < n_rows) rows[at + k] = GapRow{i, s, e};
                    });
}

// Exclusive scan of the counts in 64 bits, and the total.  One workgroup, as k_chunk_scan (kernels.hip): every thread sums a
// slab of consecutive counts, the slab sums are scanned in LDS, every thread writes its slab's bases.
__global__ __launch_bounds__(kScanThreads) void k_gap_scan(int64_t n, const uint32_t *__restrict__ counts, int64_t *__restrict__ base,
                                                           int64_t *__restrict__ total)
{
    __shared__ int64_t slab[kScanThreads];
    const int tid = threadIdx.x;
    const int64_t per = (n + kScanThreads - 1) / kScanThreads;
    const int64_t k0 = (int64_t)tid * per < n ? (int64_t)tid * per : n, k1 = k0 + per < n ? k0 + per : n;
    int64_t sum = 0;
    for (int64_t k = k0; k < k1; ++k) sum += counts[k];
    slab[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int64_t add = tid >= d ? slab[tid - d] : 0;
        __syncthreads();
        slab[tid] += add;
        __syncthreads();
    }
    int64_t run = slab[tid] - sum;
    for (int64_t k = k0; k < k1; ++k) {
        base[k] = run;
        run += counts[k];
    }
    if (tid == kScanThreads - 1) *total = slab[tid];
}

// ---- the split stage -----------------------------------------------------------------------------------------------
// the first row of the table that belongs to read i or to a later one
__device__ __forceinline__ int64_t first_gap_of(const GapRow *__restrict__ rows, int64_t n_rows, int64_t i)
{
    int64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rows[mid].read < i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A read's blocks are the non-empty stretches of [pos, end] between its gaps: with gaps g0 .. g1 - 1 (maximal, so two
// neighbours always have covered bases between them) one before the first gap unless it starts at pos, one between every
// two, one behind the last unless it ends at end.  No gap: the read itself.  All of the span a gap: none.
__device__ __forceinline__ uint32_t blocks_of(const GapRow *__restrict__ rows, int64_t g0, int64_t g1, int32_t pos, int32_t end)
{
    if (g0 == g1) return 1u;
    return (uint32_t)(rows[g0].start > pos) + (uint32_t)(g1 - g0 - 1) + (uint32_t)(rows[g1 - 1].end < end);
}

__global__ __launch_bounds__(kSpliceThreads) void k_block_count(int64_t n, const int32_t *__restrict__ pos, const int32_t *__restrict__ end,
                                                                const GapRow *__restrict__ rows, int64_t n_rows,
                                                                uint32_t *__restrict__ read_blocks, uint32_t *__restrict__ group_blocks)
{
    __shared__ uint32_t scratch[kSpliceThreads];
    const int64_t i = (int64_t)blockIdx.x * kSpliceThreads + threadIdx.x;
    uint32_t c = 0;
    if (i < n) {
        const int64_t g0 = first_gap_of(rows, n_rows, i);
        int64_t g1 = g0;
        while (g1 < n_rows && rows[g1].read == i) ++g1;
        c = blocks_of(rows, g0, g1, pos[i], end[i]);
        read_blocks[i] = c;
    }
    uint32_t total;
    bsig::block_exclusive_scan<kSpliceThreads>(c, scratch, &total);
    if (threadIdx.x == 0) group_blocks[blockIdx.x] = total;
}

// the reference of read i: the largest r < n_ref with ref_off[r] <= i (references without reads share their offset with
// the next one: the largest is the one that holds the read)
__device__ __forceinline__ int32_t ref_of(const int64_t *__restrict__ ref_off, int32_t n_ref, int64_t i)
{
    int32_t lo = 0, hi = n_ref - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (ref_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the block rows in read order: key, start, end and the read they come from; ref_row[r] = the row of reference r's first
// read (written by that read; a reference without reads keeps -1).  read_first[i] = read i's first row (read_first[n] = m)
// and read_fm[i] = its flag | mapq << 16: with bpos and bend the set's read table
__global__ __launch_bounds__(kSpliceThreads) void k_block_emit(int64_t n, int32_t n_ref, const int64_t *__restrict__ ref_off,
                                                               const int32_t *__restrict__ pos, const int32_t *__restrict__ end,
                                                               const GapRow *__restrict__ rows, int64_t n_rows,
                                                               const uint32_t *__restrict__ read_blocks, const int64_t *__restrict__ group_base,
                                                               int64_t m, uint64_t *__restrict__ key, uint32_t *__restrict__ row_id,
                                                               int32_t *__restrict__ bpos, int32_t *__restrict__ bend,
                                                               uint32_t *__restrict__ bread, long long *__restrict__ ref_row,
                                                               const uint16_t *__restrict__ flag, const uint8_t *__restrict__ mapq,
                                                               uint32_t *__restrict__ read_first, uint32_t *__restrict__ read_fm)
{
    __shared__ uint32_t scratch[kSpliceThreads];
    const int64_t i = (int64_t)blockIdx.x * kSpliceThreads + threadIdx.x;
    const uint32_t c = i < n ? read_blocks[i] : 0u;
    uint32_t total;
    const uint32_t before = bsig::block_exclusive_scan<kSpliceThreads>(c, scratch, &total);
    if (i >= n) return;
    const int64_t at = group_base[blockIdx.x] + before;
    const int32_t rid = ref_of(ref_off, n_ref, i);
    if (ref_off[rid] == i) ref_row[rid] = at;
    read_first[i] = (uint32_t)at;
    read_fm[i] = (uint32_t)flag[i] | ((uint32_t)mapq[i] << 16);
    if (i == n - 1) read_first[n] = (uint32_t)(at + c);
    if (!c) return;
    const int32_t p = pos[i], e = end[i];
    const uint64_t hi = (uint64_t)(uint32_t)rid << 32;
    uint32_t k = 0;
    auto put = [&](int32_t s, int32_t t) {
        const int64_t j = at + k;
        if (k < c && j < m) {
            key[j] = hi | ((uint32_t)s ^ 0x80000000u);       // signed order: -1 sorts before 0
            row_id[j] = (uint32_t)j;
            bpos[j] = s; bend[j] = t; bread[j] = (uint32_t)i;
        }
        ++k;
    };
    const int64_t g0 = first_gap_of(rows, n_rows, i);
    if (g0 >= n_rows || rows[g0].read != i) { put(p, e); return; }
    int32_t s = p;
    for (int64_t g = g0; g < n_rows && rows[g].read == i; ++g) {
        const GapRow r = rows[g];
        if (r.start > s) put(s, r.start - 1);
        s = r.end + 1;
        if (r.end >= e) return;          // the gap runs to the read's last base
    }
    put(s, e);
}

__global__ __launch_bounds__(kSpliceThreads) void k_block_gather(int64_t m, const uint32_t *__restrict__ order, const int32_t *__restrict__ bpos,
                                                                 const int32_t *__restrict__ bend, const uint32_t *__restrict__ bread,
                                                                 const uint16_t *__restrict__ flag, const uint8_t *__restrict__ mapq,
                                                                 const int32_t *__restrict__ tlen, int32_t *__restrict__ o_pos,
                                                                 int32_t *__restrict__ o_end, uint16_t *__restrict__ o_flag,
                                                                 uint8_t *__restrict__ o_mapq, int32_t *__restrict__ o_tlen)
{
    const int64_t k = (int64_t)blockIdx.x * kSpliceThreads + threadIdx.x;
    if (k >= m) return;
    const uint32_t j = order[k];
    const uint32_t i = bread[j];
    o_pos[k] = bpos[j];
    o_end[k] = bend[j];
    o_flag[k] = flag[i];
    o_mapq[k] = mapq[i];
    o_tlen[k] = tlen[i];
}

inline unsigned groups_of(int64_t n) { return (unsigned)((n + kSpliceThreads - 1) / kSpliceThreads); }

}  // namespace

namespace bsig {

hipError_t launch_gap_scan(int64_t n, const uint32_t *counts, int64_t *base, int64_t *total, hipStream_t st)
{
    hipLaunchKernelGGL(k_gap_scan, dim3(1), dim3(kScanThreads), 0, st, n, counts, base, total);
    return hipGetLastError();
}

int gaps_from_columns(hipStream_t st, DevPool &pool, int64_t n, const int32_t *d_pos, const uint16_t *d_flag,
                      const int64_t *d_cigar_off, const uint32_t *d_cigar, GapTable *out)
{
    *out = GapTable{};
    if (n <= 0) return BSIG_OK;
    const int64_t n_groups = groups_of(n);
    uint32_t *d_read_gaps, *d_group_gaps;
    int64_t *d_group_base, *d_total;
    HIP_TRY(pool.alloc(&d_read_gaps, (size_t)n));
    HIP_TRY(pool.alloc(&d_group_gaps, (size_t)n_groups));
    HIP_TRY(pool.alloc(&d_group_base, (size_t)n_groups));
    HIP_TRY(pool.alloc(&d_total, 1));
    hipLaunchKernelGGL(k_gap_count, dim3((unsigned)n_groups), dim3(kSpliceThreads), 0, st, n, d_pos, d_flag, d_cigar_off, d_cigar,
                       d_read_gaps, d_group_gaps);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_gap_scan(n_groups, d_group_gaps, d_group_base, d_total, st));
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (total == 0) return BSIG_OK;
    GapRow *d_rows;
    HIP_TRY(pool.alloc(&d_rows, (size_t)total));
    hipLaunchKernelGGL(k_gap_emit, dim3((unsigned)n_groups), dim3(kSpliceThreads), 0, st, n, d_pos, d_flag, d_cigar_off, d_cigar,
                       d_read_gaps, d_group_base, d_rows, total);
    HIP_TRY(hipGetLastError());
    out->rows = d_rows;
    out->n = total;
    return BSIG_OK;
}

int spliced_layout(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int32_t *ref_len, const int64_t *ref_off,
                   const int32_t *d_pos, const int32_t *d_end, const uint16_t *d_flag, const uint8_t *d_mapq,
                   const int32_t *d_tlen, const GapTable &gaps)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    R->spliced = true;
    R->rtab = bsig_reads::ReadTable{};
    R->rtab.h_ref_off.assign((size_t)std::max(n_ref, 0) + 1, 0);       // (an empty set: an empty table)
    if (n <= 0 || n_ref <= 0) {
        if (const int rc = junctions_build(ctx, R, 0, n_ref, nullptr, nullptr, nullptr, nullptr, nullptr, GapTable{})) return rc;
        return layout_from_device(ctx, R, 0, n_ref, ref_len, ref_off, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    if (n >= ((int64_t)1 << 32) - 8) return fail(BSIG_ERR_ARG, "more than 2^32 reads in a spliced set");
    DevPool tmp(2.0);
    // ---- blocks per read, their scan ------------------------------------------------------------------------------
    const int64_t n_groups = groups_of(n);
    uint32_t *d_read_blocks, *d_group_blocks;
    int64_t *d_group_base, *d_total, *d_ref_off;
    long long *d_ref_row;
    HIP_TRY(tmp.alloc(&d_read_blocks, (size_t)n));
    HIP_TRY(tmp.alloc(&d_group_blocks, (size_t)n_groups));
    HIP_TRY(tmp.alloc(&d_group_base, (size_t)n_groups));
    HIP_TRY(tmp.alloc(&d_total, 1));
    HIP_TRY(tmp.alloc(&d_ref_off, (size_t)n_ref + 1));
    HIP_TRY(tmp.alloc(&d_ref_row, (size_t)n_ref + 1));
    HIP_TRY(hipMemcpyAsync(d_ref_off, ref_off, ((size_t)n_ref + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_ref_row, 0xFF, ((size_t)n_ref + 1) * sizeof(long long), st));
    // the gaps themselves stay with the set as its junction table (junctions.hip), in the set's own pool
    if (const int rc = junctions_build(ctx, R, n, n_ref, d_ref_off, d_pos, d_end, d_flag, d_mapq, gaps)) return rc;
    hipLaunchKernelGGL(k_block_count, dim3((unsigned)n_groups), dim3(kSpliceThreads), 0, st, n, d_pos, d_end, gaps.rows, gaps.n,
                       d_read_blocks, d_group_blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_gap_scan(n_groups, d_group_blocks, d_group_base, d_total, st));
    int64_t m = 0;
    HIP_TRY(hipMemcpyAsync(&m, d_total, sizeof m, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (m >= ((int64_t)1 << 32) - 8) return fail(BSIG_ERR_ARG, "more than 2^32 aligned blocks in a spliced set");
    // ---- the rows in read order -----------------------------------------------------------------------------------
    const size_t cap = (size_t)std::max<int64_t>(m, 1);
    uint64_t *d_key, *d_key_sorted;
    uint32_t *d_row, *d_order, *d_bread;
    int32_t *d_bpos, *d_bend;
    uint32_t *d_read_first, *d_read_fm;
    int64_t *d_read_ref_off;
    HIP_TRY(tmp.alloc(&d_key, cap));
    HIP_TRY(tmp.alloc(&d_key_sorted, cap));
    HIP_TRY(tmp.alloc(&d_row, cap));
    HIP_TRY(tmp.alloc(&d_order, cap));
    HIP_TRY(tmp.alloc(&d_bread, cap));
    // the read table stays with the set: its columns come from the set's own pool, so that hbm_bytes and the cache's budget
    // count them
    HIP_TRY(R->pool.alloc(&d_bpos, cap));
    HIP_TRY(R->pool.alloc(&d_bend, cap));
    HIP_TRY(R->pool.alloc(&d_read_first, (size_t)n + 1));
    HIP_TRY(R->pool.alloc(&d_read_fm, (size_t)n));
    HIP_TRY(R->pool.alloc(&d_read_ref_off, (size_t)n_ref + 1));
    HIP_TRY(hipMemcpyAsync(d_read_ref_off, d_ref_off, ((size_t)n_ref + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_block_emit, dim3((unsigned)n_groups), dim3(kSpliceThreads), 0, st, n, n_ref, d_ref_off, d_pos, d_end, gaps.rows,
                       gaps.n, d_read_blocks, d_group_base, m, d_key, d_row, d_bpos, d_bend, d_bread, d_ref_row, d_flag, d_mapq, d_read_first,
                       d_read_fm);
    HIP_TRY(hipGetLastError());
    std::vector<long long> ref_row((size_t)n_ref + 1, -1);
    HIP_TRY(hipMemcpyAsync(ref_row.data(), d_ref_row, ref_row.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    // ---- stable sort by (reference, block start) ---------------------------------------------------------------------
    int32_t *o_pos = nullptr, *o_end = nullptr, *o_tlen = nullptr;
    uint16_t *o_flag = nullptr;
    uint8_t *o_mapq = nullptr;
    if (m > 0) {
        unsigned ref_bits = 1;
        while (ref_bits < 31 && ((int64_t)1 << ref_bits) < n_ref) ++ref_bits;
        size_t sort_bytes = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, d_key, d_key_sorted, d_row, d_order, (size_t)m, 0u, 32u + ref_bits, st));
        uint8_t *d_sort_tmp;
        HIP_TRY(tmp.alloc(&d_sort_tmp, std::max<size_t>(sort_bytes, 1)));
        HIP_TRY(rocprim::radix_sort_pairs(d_sort_tmp, sort_bytes, d_key, d_key_sorted, d_row, d_order, (size_t)m, 0u, 32u + ref_bits, st));
        HIP_TRY(tmp.alloc(&o_pos, cap));
        HIP_TRY(tmp.alloc(&o_end, cap));
        HIP_TRY(tmp.alloc(&o_tlen, cap));
        HIP_TRY(tmp.alloc(&o_flag, cap));
        HIP_TRY(tmp.alloc(&o_mapq, cap));
        hipLaunchKernelGGL(k_block_gather, dim3(groups_of(m)), dim3(kSpliceThreads), 0, st, m, d_order, d_bpos, d_bend, d_bread, d_flag,
                           d_mapq, d_tlen, o_pos, o_end, o_flag, o_mapq, o_tlen);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    // the rows of one reference stay contiguous: its first row is its first read's
    std::vector<int64_t> row_off((size_t)n_ref + 1, m);
    for (int32_t r = n_ref - 1; r >= 0; --r)
        row_off[(size_t)r] = ref_off[r] < ref_off[r + 1] && ref_row[(size_t)r] >= 0 ? (int64_t)ref_row[(size_t)r] : row_off[(size_t)r + 1];
    row_off[0] = 0;
    bsig_reads::ReadTable &T = R->rtab;
    T.n = n; T.n_blocks = m;
    T.blk_off = d_read_first; T.fm = d_read_fm; T.bstart = d_bpos; T.bend = d_bend; T.ref_off = d_read_ref_off;
    T.h_ref_off.assign(ref_off, ref_off + n_ref + 1);
    // layout_from_device synchronises the stream before it returns: tmp may be released then
    return layout_from_device(ctx, R, m, n_ref, ref_len, row_off.data(), o_pos, o_end, o_flag, o_mapq, o_tlen);
}

}  // namespace bsig

extern "C" {

int bsig_reads_upload_spliced(bsig_ctx *ctx, const bsig_columns *cols, bsig_reads **out)
{
    if (!ctx || !cols || !out) return fail(BSIG_ERR_ARG, "NULL argument to bsig_reads_upload_spliced");
    *out = nullptr;
    if (const int rc = bsig::check_columns(cols)) return rc;
    const int64_t n = cols->n_reads;
    if (n > 0 && (!cols->cigar_off || !cols->cigar))
        return fail(BSIG_ERR_ARG, "spliced reads need cigar_off + cigar: an end column does not say where the N gaps lie");
    std::unique_ptr<bsig_reads> R(new bsig_reads);
    R->ctx = ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    if (n == 0 || cols->n_ref == 0) {
        rc = bsig::spliced_layout(ctx, R.get(), 0, cols->n_ref, cols->ref_len, cols->ref_off, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  GapTable{});
    } else {
        const int64_t n_ops = cols->cigar_off[n];
        if (cols->cigar_off[0] != 0 || n_ops < 0) return fail(BSIG_ERR_ARG, "cigar_off must start at 0 and be non-decreasing");
        for (int64_t i = 0; i < n; ++i)
            if (cols->cigar_off[i] > cols->cigar_off[i + 1]) return fail(BSIG_ERR_ARG, "cigar_off must start at 0 and be non-decreasing");
        DevPool tmp;
        int32_t *d_pos, *d_end, *d_tlen;
        uint16_t *d_flag;
        uint8_t *d_mapq;
        int64_t *d_coff;
        uint32_t *d_cig;
        HIP_TRY(tmp.alloc(&d_pos, n));
        HIP_TRY(tmp.alloc(&d_end, n));
        HIP_TRY(tmp.alloc(&d_tlen, n));
        HIP_TRY(tmp.alloc(&d_flag, n));
        HIP_TRY(tmp.alloc(&d_mapq, n));
        HIP_TRY(tmp.alloc(&d_coff, n + 1));
        HIP_TRY(tmp.alloc(&d_cig, std::max<int64_t>(n_ops, 1)));
        HIP_TRY(hipMemcpyAsync(d_pos, cols->pos, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_tlen, cols->tlen, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_flag, cols->flag, n * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_mapq, cols->mapq, n * sizeof(uint8_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_coff, cols->cigar_off, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (n_ops) HIP_TRY(hipMemcpyAsync(d_cig, cols->cigar, n_ops * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        // (the end column is the CIGAR's own, whatever cols->end says: the blocks must tile [pos, end])
        HIP_TRY(bsig::launch_cigar_end(n, d_pos, d_flag, d_coff, d_cig, d_end, st));
        GapTable gaps;
        rc = bsig::gaps_from_columns(st, tmp, n, d_pos, d_flag, d_coff, d_cig, &gaps);
        if (rc == BSIG_OK)
            rc = bsig::spliced_layout(ctx, R.get(), n, cols->n_ref, cols->ref_len, cols->ref_off, d_pos, d_end, d_flag, d_mapq, d_tlen, gaps);
        if (rc != BSIG_OK) (void)hipStreamSynchronize(st);      // (tmp goes away)
    }
    if (rc != BSIG_OK) return rc;
    *out = R.release();
    return BSIG_OK;
}

int32_t bsig_reads_is_spliced(const bsig_reads *reads) { return reads && reads->spliced ? 1 : 0; }

}  // extern "C"
