// Splice junctions (junctions.hip): the gap table of a spliced set kept as a sorted resident table, and the per-range
// query over it.  Internal: not part of the C ABI.
#ifndef BSIG_JUNCTIONS_H
#define BSIG_JUNCTIONS_H
#include "filecall.h"
#include "runtime_internal.h"

namespace bsig {

struct GapTable;        // (splice_walk.h: device code, which the host-only callers of the query do not see)

// The resident junction table of R from the gap table and the read columns spliced_layout is given (device arrays; d_ref_off:
// the reads' per-reference offsets, n_ref + 1 entries): one row (start, end, flag | mapq << 16, anchor) per gap, stably
// sorted by (reference, start, end), in R's pool, with the per-reference row offsets on host and device.  Fewer than
// 2^32 - 8 gap rows.  Synchronises the stream.
int junctions_build(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int64_t *d_ref_off, const int32_t *d_pos,
                    const int32_t *d_end, const uint16_t *d_flag, const uint8_t *d_mapq, const GapTable &gaps);

// The query (bsig_reads_junctions' body): the distinct (start, end) of every range's rows that pass the filter, with their
// counts (1 value per junction, 2 with ss: sense, antisense) and largest anchors, into `out` in the caller's range order
// (columns start, end, count, max_anchor).
int junctions_query(const bsig_reads *R, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                    int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_anchor, int32_t ss, EncodedColumns *out);

// what a junction query asks of its parameters, before anything else is looked at
int junctions_rule(int32_t min_anchor);

}  // namespace bsig
struct bsig_junctions_result : bsig::EncodedColumns {
    int32_t ss = 0;
};
#endif
