// The gaps of one read: what splice.hip (CIGAR columns) and devdecode.hip (the inflated stream) share.
//
// A cursor starts at pos.  M D = X (ops 0, 2, 7, 8) advance it and are covered; N (op 3) advances it and is not; I S H P
// advance nothing.  A GAP is a maximal stretch of the read's span [pos, end] that comes from N operations: neighbouring Ns,
// and Ns separated only by I / S / H / P (or by operations of length 0), make one gap.  A read with flag 0x4 has none (it
// keeps its single row [pos, pos]); a leading or trailing N is a gap like any other.
//
// Kernels are local to the file that includes this (no relocatable device code).
#ifndef BSIG_SPLICE_WALK_H
#define BSIG_SPLICE_WALK_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bsig {

// one row of a gap table: rows are in read order, a read's gaps in the order of its CIGAR
struct GapRow {
    int64_t read;           // index of the read in its columns
    int32_t start, end;     // first and last base of the gap
};
// a gap table on the device: n rows
struct GapTable {
    const GapRow *rows = nullptr;
    int64_t n = 0;
};

// walks the n_ops operations load(q), q = 0 .. n_ops - 1 (len << 4 | op), and calls emit(k, start, end) for the k-th gap;
// returns the number of gaps.  The positions are 64-bit inside and truncated like bam_endpos - 1 is (k_bam_extract)
template <typename Load, typename Emit>
__device__ __forceinline__ uint32_t walk_gaps(int32_t pos, uint32_t flag, uint32_t n_ops, Load load, Emit emit)
{
    if (flag & 0x4u) return 0;
    int64_t cur = pos, gs = 0;
    bool open = false;
    uint32_t n = 0;
    for (uint32_t q = 0; q < n_ops; ++q) {
        const uint32_t c = load(q);
        const uint32_t op = c & 0xFu, len = c >> 4;
        if (!len) continue;
        if (op == 3u) {
            if (!open) { open = true; gs = cur; }
            cur += len;
        } else if ((0x185u >> op) & 1u) {          // bits 0, 2, 7, 8
            if (open) { emit(n, (int32_t)gs, (int32_t)(cur - 1)); ++n; open = false; }
            cur += len;
        }
    }
    if (open) { emit(n, (int32_t)gs, (int32_t)(cur - 1)); ++n; }
    return n;
}

// exclusive scan of one value per thread over a workgroup of THREADS (a power of two, <= 1024) in LDS; *total receives the
// workgroup's sum.  scratch: THREADS entries.  Every thread of the workgroup must call it.
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *scratch, uint32_t *total)
{
    const int tid = threadIdx.x;
    scratch[tid] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const uint32_t add = tid >= d ? scratch[tid - d] : 0u;
        __syncthreads();
        scratch[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = scratch[tid];
    *total = scratch[THREADS - 1];
    __syncthreads();            // (the scratch may be reused at once)
    return incl - v;
}

}  // namespace bsig
#endif
