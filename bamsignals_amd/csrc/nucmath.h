// Nucleotide counts (nucleotides.hip): what is plain arithmetic -- the channels, a read's reference span, the base table's
// size, the tiles and cells of a query.  No HIP in here: host code and sanitizer builds include it as it is; under hipcc the
// small functions are device functions as well.
#ifndef BSIG_NUCMATH_H
#define BSIG_NUCMATH_H
#include <stdint.h>

#ifdef __HIPCC__
#define BSIG_NUC_HD __host__ __device__
#else
#define BSIG_NUC_HD
#endif

namespace bsig {

constexpr int kNucChannels = 6;             // A C G T N '-'
constexpr int kNucDeletion = 5;
constexpr int32_t kNucTile = 1024;          // bases of a range one workgroup counts: 6 x 1024 int32 = 24 KB of LDS, 48 KB with ss
constexpr int32_t kNucMaxBaseQual = 93;

// the channel of a 4-bit base code: 1 -> A, 2 -> C, 4 -> G, 8 -> T, every other code -> N (one hex digit per code)
BSIG_NUC_HD inline uint32_t nuc_channel(uint32_t code) { return (uint32_t)(0x4444444344424104ull >> (4u * (code & 15u))) & 7u; }
// the channel a '-' range reports a count in: A <-> T, C <-> G; N and '-' stay
BSIG_NUC_HD inline uint32_t nuc_complement(uint32_t ch) { return ch < 4u ? 3u - ch : ch; }
// does a CIGAR operation place query bases on the reference (M = X), and does it move the two cursors?
BSIG_NUC_HD inline bool nuc_op_aligns(uint32_t op) { return ((0x181u >> op) & 1u) != 0u; }            // 0, 7, 8
BSIG_NUC_HD inline bool nuc_op_moves_ref(uint32_t op) { return ((0x18Du >> op) & 1u) != 0u; }         // 0, 2, 3, 7, 8
BSIG_NUC_HD inline bool nuc_op_moves_query(uint32_t op) { return ((0x193u >> op) & 1u) != 0u; }       // 0, 1, 4, 7, 8

// the reference bases the n_ops operations load(k) (len << 4 | op) of a read span, in 64 bits: its last base is pos + span - 1
template <typename Load>
BSIG_NUC_HD inline int64_t nuc_ref_span(int64_t n_ops, Load load)
{
    int64_t span = 0;
    for (int64_t k = 0; k < n_ops; ++k) {
        const uint32_t c = load(k);
        if (nuc_op_moves_ref(c & 15u)) span += (int64_t)(c >> 4);
    }
    return span;
}
// ... as the table keeps it: the last base, no further right than 2^31 - 1 (the window search compares with it; the walk
// itself is exact)
BSIG_NUC_HD inline int32_t nuc_clamped_end(int64_t pos, int64_t span)
{
    const int64_t e = pos + span - 1;
    return e > 0x7FFFFFFF ? 0x7FFFFFFF : e < -0x7FFFFFFF - 1 ? -0x7FFFFFFF - 1 : (int32_t)e;
}

// device bytes of a base table as its arrays are counted (not as the allocator rounds them): pos, endmax, flag | mapq << 16
// (4 each) and the two offsets (8 each, n + 1 entries) per read, 4 an operation, half a byte and a byte a base, the
// per-reference read offsets
inline int64_t nuc_table_bytes(int64_t n_reads, int64_t n_ops, int64_t n_bases, int64_t n_ref)
{
    return 12 * n_reads + 16 * (n_reads + 1) + 4 * n_ops + (n_bases + 1) / 2 + n_bases + 8 * (n_ref + 1);
}

// tiles of a range of `len` bases
inline int64_t nuc_tiles(int64_t len) { return len <= 0 ? 0 : (len + kNucTile - 1) / kNucTile; }
// cells of a range
inline int64_t nuc_cells(int64_t len, bool ss) { return len <= 0 ? 0 : (ss ? 2 : 1) * (int64_t)kNucChannels * len; }

}  // namespace bsig
#endif
