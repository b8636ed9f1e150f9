// Spliced reads (splice.hip): reads split at their N gaps into one row per aligned block, laid out as ordinary resident
// reads.  Internal: not part of the C ABI.
#ifndef BSIG_SPLICE_H
#define BSIG_SPLICE_H
#include "runtime_internal.h"
#include "splice_walk.h"

namespace bsig {

// exclusive scan of n 32-bit counts in 64 bits, and their total, on the device (one workgroup, as launch_chunk_scan)
hipError_t launch_gap_scan(int64_t n, const uint32_t *counts, int64_t *base, int64_t *total, hipStream_t st);

// The gap table of n reads from their CIGAR columns (device arrays; cigar_off has n + 1 entries).  The rows are
// allocated in `pool`; synchronises the stream (one host read sizes the table).
int gaps_from_columns(hipStream_t st, DevPool &pool, int64_t n, const int32_t *d_pos, const uint16_t *d_flag,
                      const int64_t *d_cigar_off, const uint32_t *d_cigar, GapTable *out);

// The split stage and the layout behind it: device columns of n reads in BAM order (ref_off: host, n_ref + 1) and their gap
// table -> R, a resident set whose rows are the reads' blocks, stably sorted by (reference, block start), marked spliced.
// The input columns are only read.  Fewer than 2^32 reads and block rows.
int spliced_layout(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int32_t *ref_len, const int64_t *ref_off,
                   const int32_t *d_pos, const int32_t *d_end, const uint16_t *d_flag, const uint8_t *d_mapq,
                   const int32_t *d_tlen, const GapTable &gaps);

}  // namespace bsig
#endif
