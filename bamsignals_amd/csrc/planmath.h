// The arithmetic of plan creation (runtime.hip: plan_create_impl and the *_setup functions): the tile size, the kernel
// parameters and the proofs they stand on, the tile cutter, the tiles' read loads and their 2^63 bound, the heavy split
// and the run cutters.  Plain integers and vectors: no HIP, no device, no environment -- runtime.hip reads the environment
// and passes numbers, and words every refusal itself.  tests/asan/planmath_driver.cpp includes this header and nothing
// else of the library; tests/test_planmath_cpu.py compares its answers with a numpy restatement.
#ifndef BSIG_PLANMATH_H
#define BSIG_PLANMATH_H
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/bamsignals_abi.h"
#include "bsig_types.h"
#include "host_util.h"

namespace bsig {
// bsig_params as every entry point reads them (runtime.hip: check_params)
struct PlanRule {
    int mode;               // the kernel family: BSIG_MODE_COVERAGE_EX is BSIG_MODE_COVERAGE with bins and / or strands
    bool cov_ex;            // ... that coverage (binned tiles; heavy slices watch its bins for overflow)
    int32_t binsize;        // the result's bins: profile's and coverage_ex's; 1 for coverage and count
    bool ss;                // strand-split result (profile, count, coverage_ex)
    bool mid, tspan;        // paired-end midpoint (profile, count) / extend (coverage, overlap)
    int32_t frag_len;       // a resized plan (coverage): bases every read covers from its 5' end; 0: off
    int64_t ext;            // how far beyond a range a read can count: |shift| + midpoint's tlen_filter[1], or extend's; a
                            // resized plan's frag_len - 1
    int32_t lay_binsize;    // bsig_layout's binsize (-1: count)
    int overlap;            // bamOverlaps (mode is then the count family's): 0 no, 1 type "any", 2 type "within"
    int32_t minoverlap;     // ... bases a read must share with its range (the caller's binsize field); 0 otherwise
    int threads;            // per workgroup
};
// a pair of 32-bit numbers laid out as the device's two-component vector (runtime.hip asserts it): a class's read window
// [x, y) of a tile, a run of tiles [x, y)
struct Pair32 {
    uint32_t x, y;
};
// What the plan's kind asks of its tiles (runtime.hip: PlanRequest).  All zero: a plain plan.
struct KindFacts {
    bool sum = false;               // the tiles in the order of their c0
    bool xcorr = false;             // tiles of a body and an antisense halo ...
    int32_t xcorr_body = 0;         // ... the shape's body cells (the caller's tile_cells, or the default)
    int32_t max_lag = 0;
    bool frag = false;              // count tiles whose size the caller's tile_cells sets ...
    int32_t len_bin = 0;            // ... and whose kernel divides by the row width
    int32_t own_tile_cells = 0;     // hist, summary, scaled: the shape's resolved tile_cells; these kinds' tiles are walked whole
    bool row_tiles = false;         // summary, scaled: a tile writes no cell, it carries its range's first result row
    bool capped = false;            // capped: per-base tiles whatever the result's bins (off is the RESULT's layout); a tile
                                    // carries its range's first result cell
};

// ---- tile size ------------------------------------------------------------------------------------------------------
struct TileSize {
    int cells;      // the plan's tile_cells
    int xbody;      // an xcorr plan: body cells of a tile, no wider than the widest range; else 0
};
// default tile: the widest range if it fits 2048 cells (less LDS per workgroup = more workgroups per CU), else 2048-cell
// tiles; the caller's tile_cells wins
inline TileSize tile_cells_for(const PlanRule &r, int caller_tile_cells, int64_t n, const int32_t *len, const KindFacts &kf)
{
    int64_t widest = 64;
    // (binned profiles and binned / strand-split coverage size their tiles by one rule)
    const bool binned = r.mode == BSIG_MODE_PROFILE || r.cov_ex;
    const bool split_ss = binned && r.ss;
    for (int64_t i = 0; i < n && r.mode != BSIG_MODE_COUNT; ++i)
        widest = std::max<int64_t>(widest, ((int64_t)len[i] + r.binsize - 1) / r.binsize);
    // (strand-split images hold two values per cell: keep the image at 8 KiB there too, otherwise
    // only 10 workgroups fit a CU and the launch is occupancy-bound: 0.62 -> 0.55 ms on config 4)
    const int64_t cap_cells = split_ss ? 1024 : 2048;
    int cells = caller_tile_cells > 0 ? caller_tile_cells : (int)std::min<int64_t>(widest, cap_cells);
    int min_cells = 64;
    if (binned && r.binsize > 1 && caller_tile_cells <= 0) {
        // wide bins: a tile of 2048 cells would span megabases and one wave would stream all of
        // its reads; keep a tile to about 16 kbp so that genome-wide binning still fills the chip
        const int64_t by_span = std::max<int64_t>(4, (16384 + r.binsize - 1) / r.binsize);
        cells = (int)std::min<int64_t>(cells, by_span);
        min_cells = 4;
    }
    // a tile image is at most 32 KiB of LDS
    cells = std::min(std::max(cells, min_cells), split_ss ? 4096 : 8192);
    cells = (cells + 3) & ~3;
    // cross-correlation: a body no wider than the widest range, and an image of the body and a halo of max_lag cells
    const int xbody = kf.xcorr ? (int)std::min<int64_t>(kf.xcorr_body, widest) : 0;
    if (kf.xcorr) cells = (xbody + kf.max_lag + 3) & ~3;
    // depth histogram, summaries, scaled regions: the caller's tile (16 .. 2,048 cells, checked by the kind's *_shape),
    // whatever the widest range
    if (kf.own_tile_cells > 0) cells = (kf.own_tile_cells + 3) & ~3;
    return TileSize{cells, xbody};
}

// ---- kernel parameters ----------------------------------------------------------------------------------------------
// What the parameter rules read of the resident layout (runtime.hip fills it from bsig_reads)
struct ClassFacts {
    int64_t n;              // reads in the class
    int32_t maxspan, kshift;
    bool has_p5h;           // the class has a 16-bit 5'-end column ...
    uint32_t p5h_off;       // ... which begins this many half-words behind the packed class's (0 without either)
};
struct LayoutFacts {
    ClassFacts cls[BSIG_MAX_CLASSES];
    const uint32_t *codes;  // the pair table: flag | mapq << 16 per code
    int32_t n_codes;
};
// The packed class's read bodies (SmallOne::four, CountOne::quad) take a read's offset from its chunk in signed
// 24-bit multiplies (v_mad_i32_i24: the low 24 bits of each operand, sign-extended), exact for operands in
// [-2^23, 2^23).  The operand is at most d + span - 1 + 2 |shift| + h in magnitude: d < 2^15 the position in the
// chunk, span - 1 < 256, h = |tlen| >> 1 <= tlen_filter[1] / 2 under the midpoint rule (a read outside the filter is
// forced out of every tile whatever its offset).  Wider shifts or template lengths take the full-width body.
inline bool rel24_ok(int32_t shift, bool midpoint, int32_t tf1)
{
    const int64_t h_max = midpoint ? std::max<int64_t>(0, tf1) / 2 : 0;
    const int64_t mag = shift < 0 ? -(int64_t)shift : (int64_t)shift;
    return 2 * mag + h_max + (1 << BSIG_PACK_POS_BITS) + 256 < (1ll << 23);
}
// does the flag/mapq filter reject the pair `fm` = flag | mapq << 16?  (restates fm_rejected of kernels.hip)
inline bool code_rejected(uint32_t fm, int32_t mapqual, uint32_t requiredF, uint32_t filteredF)
{
    const uint32_t nf = ~(fm & 0xFFFFu);
    return (int)((fm >> 16) & 0xFFu) < mapqual || (requiredF & nf) != 0u || (filteredF & nf) == 0u;
}
// The packed class's 16-bit 5'-end column (kernels.hip: ProfileOne::oct) serves a plan that reads nothing else of
// a packed read: bins of one base, no template-length rule, and a flag/mapq filter that rejects none of the file's
// codes (code_rejected, evaluated here on the pair table).  The half-word keeps 15 bits of the 5' end, so every
// tile's packed window must also lie in one chunk with room for a reverse read's span behind it: tile bases +
// 2 ext + maxspan + two buckets of rounding <= 2^15 - 256.  Then base + ((h - base) & 0x7FFF) is the 5' end, and
// no window has a second chunk (packed_later_chunks).  Anything else reads the 4-byte words.
inline bool packed_half_ok(const BsigKParams &K, int mode, int64_t ext, const LayoutFacts &L)
{
    const ClassFacts &C = L.cls[BSIG_CLASS_PACKED];
    bool half = mode == BSIG_MODE_PROFILE && K.binsize == 1 && !K.use_tlen && C.has_p5h;
    for (int c = 0; half && c < L.n_codes; ++c) half = !code_rejected(L.codes[c], K.mapqual, K.requiredF, K.filteredF);
    return half && (int64_t)K.tile_cells + 2 * ext + C.maxspan + 2 * ((int64_t)1 << C.kshift) <= (1 << BSIG_PACK_POS_BITS) - 256;
}
// Span classes 0 and 1 from their own 16-bit columns (kernels.hip: for_each_read under P.short_half).  Their reads'
// (flag, mapq) pairs are not the pair table's, so the filter must be one that rejects no read by its parameters
// alone: no mapq bound, no required flag, and a filtered-flag bit above the 16 a flag has (then filteredF & ~flag is
// never 0).  The window of class c for a tile holds pos in [wlo, whi) rounded outwards to buckets, wlo = tile start
// - ext - (maxspan - 1), whi = tile end + ext: at most tile bases + 2 ext + (maxspan - 1) + two buckets wide from its
// base, the rounded wlo (ProfileOne::short_base).  A reverse read's 5' end lies up to maxspan - 1 behind its pos -- or
// 255 behind it where class 0's 8-bit span field holds a span below 1, which the 256 spare bases cover.  So with
// tile bases + 2 ext + 2 (maxspan - 1) + two buckets <= 2^15 - 256 every 5' end is less than 2^15 from the base
// and base + ((h - base) & 0x7FFF) is the 5' end.  Anything else reads pos and fm as before.
// Also fills what the kernels read: where a class's column begins behind the packed class's (short_off), and ext +
// maxspan - 1 with the bucket's log2 (short_win; never 0 with the flag set: short_win[1] != 0 is the kernels' form of
// short_half)
inline bool short_half_ok(const BsigKParams &K, int64_t ext, const LayoutFacts &L, uint32_t short_off[2], int32_t short_win[2])
{
    bool sh = K.packed_half && K.mapqual <= 0 && K.requiredF == 0u && (K.filteredF >> 16) != 0u;
    for (int c = 0; sh && c < 2; ++c) {
        const ClassFacts &C = L.cls[c];
        if (C.n == 0) continue;
        sh = C.has_p5h &&
             (int64_t)K.tile_cells + 2 * ext + 2 * ((int64_t)C.maxspan - 1) + 2 * ((int64_t)1 << C.kshift) <= (1 << BSIG_PACK_POS_BITS) - 256;
    }
    for (int c = 0; c < 2; ++c) {
        const ClassFacts &C = L.cls[c];
        short_off[c] = sh && C.has_p5h ? C.p5h_off : 0u;
        short_win[c] = sh ? (int32_t)((uint32_t)(ext + (C.n ? C.maxspan - 1 : 0)) << 5 | (uint32_t)(C.n ? C.kshift : 4)) : 0;
    }
    return sh;
}
// n / binsize for 0 <= n < 2^15 as (n * m) >> s, a 24-bit multiply (binsize 2..8192; else m = s = 0):
// s = 15 + ceil(log2 b), m = ceil(2^s / b): n * m / 2^s = n / b + n * e / (b * 2^s) with e < b, and the second
// term stays below 2^-ceil(log2 b) <= 1 / b for n < 2^15, so the floor is exact; n * m < 2^32, m < 2^17
inline void div15(int32_t binsize, uint32_t *m, int32_t *s)
{
    *m = 0; *s = 0;
    if (binsize < 2 || binsize > 8192) return;
    int L = 0;
    while ((1 << L) < binsize) ++L;
    *s = 15 + L;
    *m = (uint32_t)((((uint64_t)1 << *s) + (uint64_t)binsize - 1) / (uint64_t)binsize);
}
// The kernels' parameters of a plan, all but the device pointers (ptab, overflow: runtime.hip).  overlap_quad_off:
// BAMSIGNALS_OVERLAP_QUAD=0 was set when the plan was made.
inline void fill_kparams(BsigKParams &K, const bsig_params &prm, const PlanRule &r, int tile_cells, const LayoutFacts &L,
                         const KindFacts &kf, bool overlap_quad_off)
{
    K.mapqual = prm.mapqual;
    K.requiredF = (uint32_t)prm.requiredF;
    K.filteredF = (uint32_t)prm.filteredF;
    K.has_tlen_filter = prm.n_tlen_filter == 2;
    K.tf0 = prm.tlen_filter[0]; K.tf1 = prm.tlen_filter[1];
    K.shift = r.mode == BSIG_MODE_COVERAGE ? 0 : prm.shift;
    K.midpoint = r.mid; K.tspan = r.tspan;
    K.frag_len = r.frag_len;        // (no tlen column for it: use_tlen below stays the filter's)
    K.minoverlap = r.minoverlap; K.within = r.overlap == 2;
    K.overlap_wide = r.overlap && overlap_quad_off;
    K.use_tlen = K.has_tlen_filter || r.mid || r.tspan;
    K.ss = r.ss;
    K.binsize = r.binsize;
    K.ext = (int32_t)r.ext;
    K.tile_cells = tile_cells;
    K.rel24 = rel24_ok(K.shift, r.mid, prm.tlen_filter[1]);
    K.packed_half = packed_half_ok(K, r.mode, r.ext, L) ? 1 : 0;
    K.short_half = short_half_ok(K, r.ext, L, K.short_off, K.short_win) ? 1 : 0;
    // (a frag plan's tiles are count tiles, which divide by no binsize: the multiplier is its row width's)
    magic_u31(kf.frag ? kf.len_bin : K.binsize, &K.div_magic, &K.div_shift);
    div15(K.binsize, &K.div_m15, &K.div_s15);
}

// ---- tile cutter ----------------------------------------------------------------------------------------------------
struct Tiles {
    std::vector<BsigWorkItem> items;
    bool needs_zero = false;        // some cells are reached by atomic adds, or by no tile at all
    int kernel_mode = 0;            // the kernel family that runs: a profile with wide bins runs as a bamCount
};
// count mode: bases per workgroup (with the window's reach on both sides still one chunk of the packed
// class's position bits: one index lookup per tile)
// (a frag plan's and an overlap plan's tile_cells: bases per tile, for tests of the tiles' seams)
inline int count_split_for(const PlanRule &r, int caller_tile_cells, const KindFacts &kf)
{
    const int whole = 1 << (BSIG_PACK_POS_BITS - 1);
    return (kf.frag || r.overlap) && caller_tile_cells > 0 ? std::min(std::max(caller_tile_cells, 16), whole) : whole;
}
// bins wider than a workgroup should stream on its own: every bin becomes bamCount-style
// sub-intervals that add into the (zeroed) result with integer atomics
inline bool wide_bins_for(const PlanRule &r, int caller_tile_cells, int count_split)
{
    return r.mode == BSIG_MODE_PROFILE && caller_tile_cells <= 0 && r.binsize > count_split / 2;
}
// The four shapes of a range's tiles: `w` arrives with the range's loc, len, reference and strand bit, every tile is `w`
// with its own c0, nc and out_off.
// ... the bins of a range as bamCount sub-intervals: cell c covers [c*bs, (c+1)*bs) in range orientation (ref:
// src/bamsignals.cpp:356-362), mirrored on the '-' strand
inline void wide_bin_tiles(BsigWorkItem w, bool neg, int64_t cells, int32_t binsize, int count_split, int64_t out0, int64_t mult,
                           std::vector<BsigWorkItem> &items)
{
    w.units_strand |= BSIG_ITEM_ATOMIC;
    for (int64_t c = 0; c < cells; ++c) {
        const int64_t ra = c * (int64_t)binsize, rb = std::min<int64_t>(w.len, ra + binsize);
        const int64_t g0 = neg ? w.len - rb : ra, g1 = neg ? w.len - ra : rb;
        for (int64_t a = g0; a < g1; a += count_split) {
            w.c0 = (int32_t)a;
            w.nc = (int32_t)std::min<int64_t>(count_split, g1 - a);
            w.out_off = out0 + c * mult;
            items.push_back(w);
        }
    }
}
// ... a bamCount range as sub-intervals of count_split bases; true if it was split (its tiles then add with atomics)
inline bool count_tiles(BsigWorkItem w, int count_split, int64_t out0, std::vector<BsigWorkItem> &items)
{
    const bool split = w.len > count_split;
    if (split) w.units_strand |= BSIG_ITEM_ATOMIC;
    for (int64_t a = 0; a < w.len; a += count_split) {
        w.c0 = (int32_t)a;
        w.nc = (int32_t)std::min<int64_t>(count_split, w.len - a);
        w.out_off = out0;
        items.push_back(w);
    }
    return split;
}
// ... a body of the range's cells and, behind it, as much of max_lag cells as the range still has: the tile is
// piled up over body + halo (nc) and correlated over the body, whose length rides in out_off
inline void xcorr_tiles(BsigWorkItem w, int xbody, int32_t max_lag, std::vector<BsigWorkItem> &items)
{
    for (int64_t c0 = 0; c0 < w.len; c0 += xbody) {
        const int64_t nb = std::min<int64_t>(xbody, w.len - c0);
        w.c0 = (int32_t)c0;
        w.nc = (int32_t)(nb + std::min<int64_t>(max_lag, w.len - c0 - nb));
        w.out_off = nb;
        items.push_back(w);
    }
}
// ... tile_cells cells at a time; a tile's out_off is its first cell's, out0 + c0 * step (step 0: the range's row)
inline void cell_tiles(BsigWorkItem w, int64_t cells, int tile_cells, int64_t out0, int64_t step, std::vector<BsigWorkItem> &items)
{
    for (int64_t c0 = 0; c0 < cells; c0 += tile_cells) {
        w.c0 = (int32_t)c0;
        w.nc = (int32_t)std::min<int64_t>(tile_cells, cells - c0);
        w.out_off = out0 + c0 * step;
        items.push_back(w);
    }
}
// The ranges cut into tiles, in the order `order` (genomic: neighbouring workgroups then stream neighbouring reads).  off:
// bsig_layout's n + 1 offsets; ref_unit0 / ref_units: per reference.
inline Tiles cut_tiles(const std::vector<int64_t> &order, const int32_t *rid, const int32_t *loc, const int32_t *len,
                       const int32_t *strand, const int64_t *off, const uint32_t *ref_unit0, const uint32_t *ref_units,
                       const PlanRule &r, int caller_tile_cells, const TileSize &ts, const KindFacts &kf)
{
    Tiles T;
    T.items.reserve(order.size());
    const int64_t mult = r.ss ? 2 : 1;
    const int count_split = count_split_for(r, caller_tile_cells, kf);
    const bool wide_bins = wide_bins_for(r, caller_tile_cells, count_split);
    T.kernel_mode = wide_bins ? BSIG_MODE_COUNT : r.mode;
    for (const int64_t i : order) {
        if (len[i] <= 0) {
            if (off[i + 1] > off[i]) T.needs_zero = true;      // bamCount of a zero-width range: 0
            continue;
        }
        BsigWorkItem w{};
        w.loc = loc[i]; w.len = len[i];
        w.ref_unit0 = ref_unit0[rid[i]];
        w.units_strand = ref_units[rid[i]] | (strand[i] < 0 ? BSIG_ITEM_NEG : 0u);
        const int64_t cells = kf.capped ? (int64_t)len[i] : (off[i + 1] - off[i]) / mult;
        if (kf.capped) {
            cell_tiles(w, cells, ts.cells, off[i], 0, T.items);
        } else if (wide_bins) {
            wide_bin_tiles(w, strand[i] < 0, cells, r.binsize, count_split, off[i], mult, T.items);
            T.needs_zero = true;
        } else if (r.mode == BSIG_MODE_COUNT) {
            if (count_tiles(w, count_split, off[i], T.items)) T.needs_zero = true;
        } else if (kf.xcorr) {
            xcorr_tiles(w, ts.xbody, kf.max_lag, T.items);
        } else if (kf.row_tiles) {
            cell_tiles(w, cells, ts.cells, i * mult, 0, T.items);
        } else {
            cell_tiles(w, cells, ts.cells, off[i], mult, T.items);
        }
    }
    // a sum plan adds up all tiles of one c0 (every range has the same width, so also the same nc): consecutive
    if (kf.sum) std::stable_sort(T.items.begin(), T.items.end(), [](const BsigWorkItem &a, const BsigWorkItem &b) { return a.c0 < b.c0; });
    return T;
}

// ---- capped 5' ends -------------------------------------------------------------------------------------------------
// The bins of a capped plan's result as its kernel divides: the caller's binsize, and for bamCount (lay_binsize -1) one bin
// of 2^31 - 1 bases, wider than any range
inline int32_t capped_binsize(int32_t lay_binsize) { return lay_binsize < 0 ? INT32_MAX : lay_binsize; }
// The bins a tile of at most tile_cells per-base cells can touch: cells c0 .. c0 + tile_cells - 1 with c0 anywhere in a bin
// lie in at most (tile_cells - 1) / binsize + 2 consecutive bins (floor((c0 + n - 1) / b) - floor(c0 / b) <= (n - 1) / b + 1,
// counted inclusively).  The int32 LDS accumulators a row of k_capped_tiles; 0 for bins of one base, which have none.
inline int32_t capped_tile_bins(int32_t tile_cells, int32_t binsize)
{
    if (binsize <= 1 || tile_cells < 1) return 0;
    return (int32_t)(((int64_t)tile_cells - 1) / binsize + 2);
}
// The capped coverage's stage 1 piles the capped 5' ends up over every range widened by frag_len - 1 bases on both sides: a
// read covers frag_len bases from its 5' end, so ends that far outside still reach the range.  The left end is clipped at
// base 0 -- nothing has a 5' end below it, the clipped part counts as zeros; a range that begins below 0 loses its own bases
// below 0 too, which no read covers (lead is then negative) --; the right end is left to overhang the reference.
struct CappedWide {
    int32_t loc, len;       // the widened range (len 0 for a range without width, or with nothing at or above base 0)
    int32_t lead;           // bases of it in front of the range's own first base: at most frag_len - 1; negative: the range's
                            // first -lead bases lie below base 0
    bool fits;              // false: the widened range's end passes 2^31 - 1
};
inline CappedWide capped_widen(int32_t loc, int32_t len, int32_t frag_len)
{
    CappedWide c{loc, 0, 0, true};
    if (len <= 0) return c;
    const int64_t lo = std::max<int64_t>((int64_t)loc - (frag_len - 1), 0);
    const int64_t lead = (int64_t)loc - lo;
    const int64_t wide = lead + (int64_t)len + (frag_len - 1);
    c.fits = wide <= INT32_MAX && lo + wide <= INT32_MAX;
    if (!c.fits) return c;
    c.lead = (int32_t)lead;
    if (wide <= 0) return c;
    c.loc = (int32_t)lo; c.len = (int32_t)wide;
    return c;
}
// k_capped_cover's indexes into a scratch row of inclusive prefix sums (PF of the forward ends, PR of the reverse ends; an
// index below 0 reads as 0): the coverage of the range's base u (genome order, 0-based) is
//   PF[u + lead] - PF[u + lead - L]  +  PR[u + lead + L - 1] - PR[u + lead - 1]
// -- the forward reads with their 5' end in [u - L + 1, u], the reverse reads with theirs in [u, u + L - 1] --, and 0 where
// u + lead < 0: that base lies below base 0, where no read is.
struct CappedIdx {
    int64_t f_hi, f_lo, r_hi, r_lo;
};
inline CappedIdx capped_window(int32_t u, int32_t lead, int32_t frag_len)
{
    const int64_t j = (int64_t)u + lead;
    return CappedIdx{j, j - frag_len, j + frag_len - 1, j - 1};
}

// ---- tile loads, bounds, heavy split --------------------------------------------------------------------------------
// the reads in every tile's windows (win: BSIG_MAX_CLASSES index ranges a tile, k_resolve_tiles' output)
inline std::vector<int64_t> reads_of_tiles(const std::vector<Pair32> &win)
{
    std::vector<int64_t> reads(win.size() / BSIG_MAX_CLASSES);
    for (size_t t = 0; t < reads.size(); ++t) {
        int64_t total = 0;
        for (int c = 0; c < BSIG_MAX_CLASSES; ++c) total += (int64_t)win[t * BSIG_MAX_CLASSES + c].y - win[t * BSIG_MAX_CLASSES + c].x;
        reads[t] = total;
    }
    return reads;
}
// What the cells of tiles [a, b) can add up to: a read in a tile's windows adds at most 1 to one cell of the tile (5' ends)
// or to each of its cells (coverage).  The depth histogram's bound over all tiles, the summaries' over a range's own.
inline long double depth_bound(const std::vector<BsigWorkItem> &items, const std::vector<int64_t> &reads, size_t a, size_t b, bool coverage)
{
    long double bound = 0;
    for (size_t t = a; t < b; ++t) bound += coverage ? (long double)reads[t] * (long double)items[t].nc : (long double)reads[t];
    return bound;
}
constexpr long double kTwo63 = 9223372036854775808.0L;
// The cross-correlation's bound.  A tile with n reads in its windows counts each of them in at most one cell, so
// sum(S) + sum(A) <= n and every sum the tile adds to -- a lag's S[x] A[x + d], a strand's squares -- is at most n^2.
// The tiles that are not heavy have n <= 2^15; the heavy ones' n is known (split_heavy: heavy_sq).
inline long double xcorr_bound(int64_t n_items, int64_t n_heavy_tiles, long double heavy_sq)
{
    return (long double)(n_items - n_heavy_tiles) * 1073741824.0L + heavy_sq;
}
// One wave streams a tile's reads; a tile on a read hotspot (chrM, rDNA, an amplicon) can hold millions and would keep the
// whole launch waiting.  A tile with more than heavy_reads reads is heavy: it gets BSIG_ITEM_HEAVY and its reads are
// piled up by items of a second launch --
//   kSlice: its class windows cut into slices of slice_reads that separate workgroups add up with atomics (in count mode
//           the slices carry BSIG_ITEM_ATOMIC): a slice item has one non-empty class window, in hwin;
//   kWalkWhole: the tile itself, walked by one workgroup into an image of 32-bit cells, no windows: where a cell's value
//           must be complete before it is counted or compared (hist, summary, scaled: a max is not linear in slices of
//           the reads) or multiplied (xcorr: a product of two counts is not either).
enum HeavyPolicy { kSlice, kWalkWhole };
struct HeavySplit {
    std::vector<BsigWorkItem> hitems;
    std::vector<Pair32> hwin;       // kSlice: BSIG_MAX_CLASSES windows per slice item
    int64_t n_heavy_tiles = 0;
    long double heavy_sq = 0;       // the squares of the heavy tiles' read counts, summed (xcorr_bound)
};
inline HeavySplit split_heavy(std::vector<BsigWorkItem> &items, const std::vector<Pair32> &win, const std::vector<int64_t> &reads,
                              int64_t heavy_reads, int64_t slice_reads, HeavyPolicy policy, bool count_mode)
{
    HeavySplit H;
    for (size_t t = 0; t < items.size(); ++t) {
        const int64_t total = reads[t];
        if (total <= heavy_reads) continue;
        ++H.n_heavy_tiles;
        H.heavy_sq += (long double)total * (long double)total;
        if (policy == kWalkWhole) {
            H.hitems.push_back(items[t]);
        } else {
            BsigWorkItem sl = items[t];
            if (count_mode) sl.units_strand |= BSIG_ITEM_ATOMIC;
            for (int c = 0; c < BSIG_MAX_CLASSES; ++c) {
                const Pair32 wc = win[t * BSIG_MAX_CLASSES + c];
                for (int64_t j0 = wc.x; j0 < (int64_t)wc.y; j0 += slice_reads) {
                    H.hitems.push_back(sl);
                    for (int k = 0; k < BSIG_MAX_CLASSES; ++k)
                        H.hwin.push_back(k == c ? Pair32{(uint32_t)j0, (uint32_t)std::min<int64_t>(j0 + slice_reads, wc.y)} : Pair32{0u, 0u});
                }
            }
        }
        items[t].units_strand |= BSIG_ITEM_HEAVY;
    }
    return H;
}

// ---- run cutters ----------------------------------------------------------------------------------------------------
// The plan's tiles, in their order, cut into runs of at most `per` tiles whose weights add up to `ceiling` at most (a tile
// heavier than the ceiling makes a run of its own)
template <typename Weight>
inline void cut_runs(int64_t n_items, int64_t per, int64_t ceiling, Weight &&weight, std::vector<Pair32> &runs)
{
    int64_t a = 0, in_run = 0;
    for (int64_t t = 0; t < n_items; ++t) {
        const int64_t w = weight(t);
        if (t > a && (t - a >= per || in_run + w > ceiling)) {
            runs.push_back(Pair32{(uint32_t)a, (uint32_t)t});
            a = t; in_run = 0;
        }
        in_run += w;
    }
    if (a < n_items) runs.push_back(Pair32{(uint32_t)a, (uint32_t)n_items});
}
// the wide tiles (32-bit image) follow the main runs as runs of one tile each: they are few and long
inline void append_wide_runs(int64_t n_wide, std::vector<Pair32> &runs)
{
    for (int64_t k = 0; k < n_wide; ++k) runs.push_back(Pair32{(uint32_t)k, (uint32_t)k + 1u});
}
// A sum plan's tiles (ordered by c0): the tiles of one c0 cut into runs of at most `per` (a workgroup each, one slab each),
// and the runs' slabs into chunks of at most kSumChunkSlots slabs of one c0 for k_sum_reduce.  Appends to runs and chunks
// (the heavy slices' follow the main tiles'); S: values per cell.  Returns the most values a run's slab holds.
constexpr int64_t kSumChunkSlots = 32;
inline int32_t cut_sum_runs(const std::vector<BsigWorkItem> &it, int64_t per, int32_t S, std::vector<Pair32> &runs,
                            std::vector<BsigSumChunk> &chunks)
{
    int32_t max_nvals = 0;
    int64_t chunk_c0 = -1;
    for (size_t a = 0; a < it.size();) {
        size_t b = a;
        while (b < it.size() && it[b].c0 == it[a].c0) ++b;             // the tiles of one c0: [a, b)
        for (size_t r = a; r < b; r += (size_t)per) {
            const uint32_t slot = (uint32_t)runs.size();
            runs.push_back(Pair32{(uint32_t)r, (uint32_t)std::min<size_t>(b, r + (size_t)per)});
            if (chunk_c0 != it[a].c0 || chunks.back().slot_hi - chunks.back().slot_lo >= kSumChunkSlots) {
                chunks.push_back(BsigSumChunk{slot, slot, it[a].c0 * S, it[a].nc * S});
                chunk_c0 = it[a].c0;
            }
            chunks.back().slot_hi = slot + 1;
            max_nvals = std::max(max_nvals, it[a].nc * S);
        }
        a = b;
    }
    return max_nvals;
}
}  // namespace bsig
#endif
