// Structures shared by the host runtime and the gfx950 kernels.
//
// HBM layout of the reads (built once per BAM by the prep kernels):
//   * reads are split by reference span into "span classes" (span <= 256 | <= 4096 | <= 65536 |
//     longer = classes 0..3), and the short ones (span <= 256) once more: those whose (flag, mapq)
//     pair is one of the file's BSIG_PACK_CODES most frequent pairs form the PACKED class
//     (BSIG_CLASS_PACKED), ONE 32-bit word per read
//        word : pos & 0x7FFF | (span - 1) << 15 | code << 23
//     -- a read window is narrower than 32,768 bases (wider ones are walked in chunks of that
//     width), so the low 15 bits of pos and the window's start give pos back; `code` indexes the
//     file's pair table fmtab[code] = flag | mapq << 16.  The filter on flag and mapq
//     (src/bamsignals.cpp:328-331) is evaluated once per code and launch, not once per read.
//     Short reads with a rarer pair, with flag bits above the 12 SAM defines or with pos outside
//     their reference stay in class 0.  Inside a class reads keep BAM order
//     (sorted by reference id, then pos).  Classes 0..3 have 32-bit columns
//        pos  : 0-based leftmost position                         (core.pos)
//        end  : bam_endpos - 1, inclusive                         (src/bamsignals.cpp:16-18)
//               -- classes 2..3 only; classes 0 and 1 keep span - 1 inside fm
//        fm   : class 0 (span <= 256):  flag | mapq << 16 | (span - 1) << 24
//               class 1 (span <= 4096, flag < 4096): flag | mapq << 12 | (span - 1) << 20
//               classes 2..3: flag | mapq << 16
//        tlen : template length                                   (core.isize)
//     The packed class has one more column, derived from fm and fmtab when the reads are made and never saved:
//        p5h  : (5' end & 0x7FFF) | reverse << 15, 16 bits  (5' end = pos, or pos + span - 1 on the reverse strand)
//     -- all a per-base profile without a template-length rule reads of a packed read when the plan's flag/mapq
//     filter rejects none of the file's codes (bsig_plan_create: BsigKParams::packed_half).
//     Classes 0 and 1 have the same column beside pos and fm, at the same read index (span - 1 from fm >> 24 and
//     fm >> 20, the strand from flag bit 0x10), for the same plans when the filter can reject no read whatever its
//     flag and mapq (BsigKParams::short_half): 2 bytes a visit instead of 8.  A class that holds a read with pos
//     outside its reference has none: the index files such a read under a bucket its position does not lie in.
//     and a bucket index  idx[b] = first read of the class whose global coordinate
//     g = (ref_unit0[rid] << 16) + pos  falls in bucket >= b, bucket = g >> kshift.
//     References are laid out back to back in units of 64 kbp, so one flat index
//     serves every reference.
//   * splitting by span bounds the left extension of a range's candidate window by the
//     class's own maximum span: one 2 kb intron-spanning read does not widen the window
//     of the 100-bp reads.
#ifndef BSIG_TYPES_H
#define BSIG_TYPES_H
#include <stdint.h>

#define BSIG_MAX_CLASSES 5
#define BSIG_SPAN_CLASSES 4      // classes 0..3: by span
#define BSIG_CLASS_PACKED 4      // span <= 256 and a frequent (flag, mapq) pair: one word per read (in .fm)
#define BSIG_PACK_POS_BITS 15    // low bits of pos kept in a packed word = log2 of a window chunk
#define BSIG_PACK_CODES 512      // entries of the pair table (9-bit codes)
#define BSIG_REF_UNIT_SHIFT 16   // references are laid out in units of 65536 bp

struct BsigClassCols {
    const int32_t *pos;
    const int32_t *end;
    const uint32_t *fm;
    const int32_t *tlen;
    const uint16_t *p5h;     // packed class and classes 0, 1 (NULL elsewhere, with BAMSIGNALS_PACKED_HALF=0, and for classes
                             // 0, 1 with BAMSIGNALS_SHORT_HALF=0 or a read outside its reference): see above
    const uint32_t *idx;     // n_buckets + 1 entries
    int64_t n;               // reads in the class
    int32_t maxspan;         // max(end - pos + 1) over the class
    int32_t kshift;          // log2(bucket width in bp)
};

struct BsigReadsDev {
    BsigClassCols cls[BSIG_MAX_CLASSES];
    const uint32_t *fmtab;   // BSIG_PACK_CODES entries: flag | mapq << 16 of a packed word's code (zero-padded)
    int32_t n_codes;         // codes in use
};

// One unit of GPU work: a tile of at most `tile_cells` output cells of one range
// (the device-side analogue of GArray, src/bamsignals.cpp:32-50).
struct BsigWorkItem {
    int32_t loc;        // range start, 0-based
    int32_t len;        // range width
    int32_t c0;         // profile/coverage: first cell of the tile (range orientation)
                        // count: first base of the sub-interval, relative to loc
    int32_t nc;         // profile/coverage: cells in the tile; count: bases in the sub-interval
    int64_t out_off;    // flat int32 offset of the tile's first output cell
    uint32_t ref_unit0; // first 64-kbp unit of the range's reference in the global coordinate
    uint32_t units_strand;  // BSIG_ITEM_* bits below
};
#define BSIG_ITEM_UNITS_MASK 0x0FFFFFFFu   // 64-kbp units of the range's reference
#define BSIG_ITEM_HEAVY (1u << 29)         // its reads are piled up by slice items of a second launch
#define BSIG_ITEM_NEG (1u << 30)           // range is on the '-' strand
#define BSIG_ITEM_ATOMIC (1u << 31)        // count mode: add with a global atomic (range was split)

// What the index says about one tile (k_resolve_tiles -> the pileup kernels of a large launch): the read
// windows of the five classes, and the packed class's first chunk
struct BsigResolved {
    uint32_t win[2 * BSIG_MAX_CLASSES];   // [j_lo, j_hi) per class
    int32_t pbase, pchunks;
};

struct BsigKParams {
    int32_t mapqual;
    uint32_t requiredF;
    uint32_t filteredF;
    int32_t has_tlen_filter;
    int32_t tf0, tf1;
    int32_t use_tlen;       // tlen column needed (filter, midpoint or tspan)
    int32_t shift;
    int32_t midpoint;
    int32_t tspan;
    int32_t ss;
    int32_t binsize;        // >= 1 (profile, binned coverage; 1 for per-base coverage)
    uint32_t div_magic;     // exact n / binsize for 0 <= n < 2^31:
    int32_t div_shift;      //   __umulhi(n, div_magic) >> div_shift        (binsize >= 2)
    uint32_t div_m15;       // ... and for 0 <= n < 2^15 (a range shorter than 32,768 bases) at the full rate of the
    int32_t div_s15;        //   vector unit: (n * div_m15) >> div_s15, a 24-bit multiply (binsize 2..8192; else 0)
    int32_t rel24;          // 1: the packed class's read bodies may take a read's offset from its chunk in 24-bit
                            //   multiplies (|2 shift| + tlen_filter[1] / 2 small enough: see bsig_plan_create); 0: they
                            //   take the full-width per-read body instead
    int32_t packed_half;    // 1: the packed class is read from its 16-bit 5'-end column p5h (bamProfile, binsize 1, no
                            //   template-length rule, no code rejected, every packed window one chunk: bsig_plan_create)
    int32_t short_half;     // 1: ... and so are span classes 0 and 1, from theirs (packed_half, a flag/mapq filter that can
                            //   reject no read at all, each class's window inside 2^15 bases: bsig_plan_create).  The HOST's
                            //   record of the decision (stats); the kernels do not read it, they ask short_win[1] != 0
    uint32_t short_off[2];  // ... where class 0's and 1's columns begin, in half-words from the packed class's (one block
                            //   holds the three; multiples of 8, so the columns are 16-B aligned)
    int32_t short_win[2];   // ... (ext + maxspan - 1) << 5 | kshift of class 0 and 1: where the class's window of a tile
                            //   begins.  0 without short_half and never 0 with it (kshift >= 4; an empty class gets 4):
                            //   short_win[1] is the flag the kernels branch on
    int32_t ext;            // window extension on both sides (src/bamsignals.cpp:457,487)
    int32_t tile_cells;     // output cells per tile (sizes the dynamic LDS image)
    int32_t accumulate;     // 1: add the tile image into the result with integer atomics (slices of
                            // a heavy tile) instead of storing it
    int32_t resolved;       // 1: `windows` holds one BsigResolved per tile, written by k_resolve_tiles in
                            // front of this launch (large launches: the tile's item and its windows then
                            // arrive in ONE memory round trip instead of two dependent ones)
    int32_t cov_reps;       // binned coverage: copies of the tile image (set by the launch, see k_coverage_bins)
    const uint8_t *ptab;    // the packed class's filter table for THESE parameters (BSIG_PACK_CODES bytes on the
                            // device: bit 0 rejected, bit 1 reverse strand), made once per plan by k_make_ptab
    int32_t *overflow;      // binned coverage: set to 1 by a heavy tile's slice whose atomic add took a bin past
                            // INT32_MAX (the plan's device flag; NULL where no add can)
    int32_t minoverlap;     // bamOverlaps (k_overlap*): bases a read must share with its range, >= 1; 0: no overlap plan
    int32_t within;         // ... 1: and the read must lie inside the range (type "within")
    int32_t overlap_wide;   // ... 1: packed reads take the per-read 64-bit body too, not OverlapOne::quad's 32-bit one
                            //   (BAMSIGNALS_OVERLAP_QUAD=0 at plan time: what scripts/overlaps_times.py compares)
    int32_t frag_len;       // bamCoverage of a resized plan (bsig_plan_create_resized): every read covers exactly this many
                            //   bases from its 5' end in its own direction (kernels.hip: covered_interval); 0: off.  Never
                            //   set together with tspan; asks for no tlen column (use_tlen stays the filter's)
};

// Sums over ranges (kernels.hip: k_sum_reduce): slabs [slot_lo, slot_hi) of runs of one tile position, added into the
// per-base sums from value cell0 (= c0 * S) on, nvals (= nc * S) of them; at most kSumChunkSlots slabs a chunk
struct BsigSumChunk {
    uint32_t slot_lo, slot_hi;
    int32_t cell0, nvals;
};

// Capped coverage (capped.hip: k_capped_scan, k_capped_cover): one range's row of the scratch -- the capped per-base 5' ends
// of the range widened by frag_len - 1 on both sides, (forward, reverse) pairs in genome order -- and its cells of the result
struct BsigCappedRange {
    int64_t s_off;      // int32 offset of the row in the scratch (even: a pair is 8-B aligned)
    int64_t r_off;      // int32 offset of the range's first result cell (bsig_layout)
    int32_t w;          // the range's width
    int32_t lead;       // pairs in front of the range's first base: frag_len - 1, less what lies below base 0 (negative: so
                        // many of the range's own first bases lie below base 0)
    int32_t slen;       // pairs in the row: lead + w + frag_len - 1 (0 for a range without width)
    int32_t neg;        // 1: range on the '-' strand
};

#endif
