// Nucleotide counts (nucleotides.hip): the base table a set with bases keeps beside its resident reads, and the per-range
// A / C / G / T / N / deletion counts counted from it.  Internal: not part of the C ABI.
#ifndef BSIG_NUCLEOTIDES_H
#define BSIG_NUCLEOTIDES_H
#include "nucmath.h"
#include "runtime_internal.h"

namespace bsig {

// what a nucleotide query asks of its parameters, before anything else is looked at
int nucleotides_rule(int32_t min_base_qual);

// The base table of R from host columns of n reads in BAM order (cigar_off + cigar, the three arrays of `bases`): the
// arrays go into R's own pool, R is marked has_bases.  n == 0 or no references: an empty table.  Synchronises the stream.
int bases_from_columns(bsig_ctx *ctx, bsig_reads *R, const bsig_columns *cols, const bsig_base_columns *bases);

// What one chunk of an inflated stream leaves of its records' bases (devdecode.hip: chunk_bases), all on the device and numbered
// within the chunk: read k of the chunk owns operations cig_off[k] .. and bases seq_off[k] .. (its successor's offset, or the
// chunk's total, closes it); base g of the chunk is nibble g of seq and byte g of qual
struct BasePiece {
    int64_t n = 0, n_ops = 0, n_bases = 0;
    const int64_t *cig_off = nullptr, *seq_off = nullptr;     // n entries each
    const uint32_t *cigar = nullptr;
    const uint8_t *seq = nullptr, *qual = nullptr;
};
// The base table of R from a device decode: the chunks' pieces put one behind the other in R's own pool (a piece that begins on
// an odd nibble is shifted into place), pos copied, endmax and flag | mapq << 16 made on the host from the downloaded end,
// flag and mapq columns.  d_pos .. d_mapq: the n reads' device columns in BAM order; ref_off: host, n_ref + 1.  Synchronises.
int bases_from_device(bsig_ctx *ctx, bsig_reads *R, int64_t n, int32_t n_ref, const int64_t *ref_off, const int32_t *d_pos,
                      const int32_t *d_end, const uint16_t *d_flag, const uint8_t *d_mapq, const std::vector<BasePiece> &pieces);

// The query (the body of bsig_reads_nucleotides and of the file-level call): the cells of every range, in the caller's range
// order, into device memory (out_dev) or host memory (out_host) -- exactly one of the two
int nucleotides_query(const bsig_reads *R, int64_t n, const int32_t *rid, const int32_t *loc, const int32_t *len, const int32_t *strand,
                      int32_t mapqual, int32_t requiredF, int32_t filteredF, int32_t min_base_qual, int32_t ss, int32_t *out_dev,
                      int32_t *out_host);

}  // namespace bsig
#endif
